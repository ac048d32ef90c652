// C ABI of libctc_amd.so (see include/ctc_amd.h for the contract of every entry point).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ctc_align_long.h"
#include "ctc_align_long_wild.h"
#include "ctc_align_wild.h"
#include "ctc_amd.h"
#include "ctc_beam.h"
#include "ctc_common.h"
#include "ctc_edit_long_plan.h"
#include "ctc_hvp_fused.h"
#include "ctc_launch.h"
#include "ctc_loss_long.h"
#include "ctc_nbest_align.h"
#include "ctc_prefix.h"
#include "ctc_wild_loss.h"

namespace ctc {
// diagnostic override read by ctc_hessian.hip (ctc_amd_debug_override): process-wide, written only by tests / benchmarks between calls
int g_force_hessian_slab = 0;  // 1 = the general one-slab-per-wavefront Hessian kernel also for short labels
}  // namespace ctc

namespace {

using ctc::Layout;
using ctc::Problem;

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int hip_fail(hipError_t e, const char *where) { return fail(CTC_AMD_EHIP, "%s: %s", where, hipGetErrorString(e)); }

#define CTC_TRY(launch, where) do { const hipError_t e_ = (launch); if (e_ != hipSuccess) return hip_fail(e_, where); } while (0)

// Limits (include/ctc_amd.h "Limits"): CTC_AMD_EINVAL beyond them
constexpr int MAX_U = CTC_AMD_MAX_U;            // scan_kernel is instantiated for up to 16 label positions per lane
constexpr int MAX_V_GRAD = CTC_AMD_MAX_V;       // one LDS token row per wavefront (64 KB)
constexpr int MAX_V_HESS = CTC_AMD_MAX_V_HESSIAN;  // the Hessian / HVP kernels keep V + 4 floats of LDS per wavefront

// ---- arguments ----

struct Common {  // what every compute entry point takes first
  int kind, wrt;
  const void *logits;
  const int32_t *labels;
  int label_stride;
  const int32_t *label_length, *logit_length;
  int blank, B, T, V, U;
};

// the guard of the query functions, which take a shape and no tensors (max_u: as in check_common)
bool shape_ok(int kind, int B, int T, int V, int U, int max_u = MAX_U) {
  return (kind == CTC_AMD_CLASSIC || kind == CTC_AMD_SIMPLIFIED) && B >= 0 && T >= 0 && V > 0 && U >= 0 && U <= max_u;
}

int check_common(const Common &c, int max_u = MAX_U) {  // (max_u: CTC_AMD_LONG_MAX_U for the tiled alignment, whose label axis spans workgroups)
  if (c.kind != CTC_AMD_CLASSIC && c.kind != CTC_AMD_SIMPLIFIED) return fail(CTC_AMD_EINVAL, "kind must be 0 (classic) or 1 (simplified), got %d", c.kind);
  if (c.wrt != CTC_AMD_WRT_LOGITS && c.wrt != CTC_AMD_WRT_LOGPROBS) return fail(CTC_AMD_EINVAL, "wrt must be 0 (logits) or 1 (logprobs), got %d", c.wrt);
  if (c.B < 0 || c.T < 0 || c.V <= 0 || c.U < 0 || c.label_stride < 0)
    return fail(CTC_AMD_EINVAL, "negative size: B=%d T=%d V=%d U=%d label_stride=%d", c.B, c.T, c.V, c.U, c.label_stride);
  if (c.blank < 0 || c.blank >= c.V) return fail(CTC_AMD_EINVAL, "blank_index %d outside [0, %d)", c.blank, c.V);
  if (c.U > max_u) return fail(CTC_AMD_EINVAL, "U=%d exceeds the supported maximum %d", c.U, max_u);
  if (c.B > 0 && (!c.label_length || !c.logit_length)) return fail(CTC_AMD_EINVAL, "null length pointer");
  if (c.B > 0 && c.T > 0 && !c.logits) return fail(CTC_AMD_EINVAL, "null logits pointer");
  if (c.B > 0 && c.label_stride > 0 && !c.labels) return fail(CTC_AMD_EINVAL, "null labels pointer");
  if (c.B > 65535 * 32767) return fail(CTC_AMD_EINVAL, "B too large");
  return CTC_AMD_OK;
}

int low_bits(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr) {
  return (int)((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15);
}

// contiguous float32 [B,T,V] logits and gradient until a Format says otherwise
Problem make_problem(const Common &c) {
  Problem p;
  p.logits = static_cast<const float *>(c.logits);  // element-typed inside the kernels (Problem::xdtype)
  p.labels = c.labels; p.label_length = c.label_length; p.logit_length = c.logit_length;
  p.label_stride = c.label_stride; p.blank = c.blank; p.B = c.B; p.T = c.T; p.V = c.V; p.U = c.U; p.kind = c.kind; p.wrt = c.wrt;
  p.xsb = (long)c.T * c.V; p.xst = c.V; p.gsb = (long)c.T * c.V; p.gst = c.V; p.xdtype = 0; p.gdtype = 0;
  p.align_bits = low_bits(c.logits);  // (entry points OR in the tensors they write)
  return p;
}

Problem shape_problem(int kind, int wrt, int B, int T, int V, int U) {  // what a contiguous float32 call of this shape would run
  return make_problem(Common{kind, wrt, nullptr, nullptr, 0, nullptr, nullptr, 0, B, T, V, U});
}

// Producer formats (ctc_amd_loss_grad_ex and its kin): element types and element strides of the batch and time axes of the
// logits (x) and of the gradient (g); the token axis is contiguous.  Packed batches have rows and no batch stride (sb = 0):
// utterance b starts at row row0[b].
struct Format {
  int xdtype;
  int64_t xsb, xst;
  int gdtype;
  int64_t gsb, gst;
  bool packed = false;
  const int64_t *row0 = nullptr;
  // a call without a gradient of its own: the pipeline is chosen as for a gradient in the logits' format
  static Format of_logits(int dtype, int64_t sb, int64_t st) { return {dtype, sb, st, dtype, sb, st}; }
  int check_dtypes() const {
    if (xdtype < CTC_AMD_F32 || xdtype > CTC_AMD_F16 || gdtype < CTC_AMD_F32 || gdtype > CTC_AMD_F16)
      return fail(CTC_AMD_EINVAL, "dtype must be CTC_AMD_F32, CTC_AMD_BF16 or CTC_AMD_F16 (logits %d, grad %d)", xdtype, gdtype);
    return CTC_AMD_OK;
  }
  // rows must not overlap: stride_t >= V, and the batch stride must step over whole rows in either nesting order
  int check_strides(int V, bool with_grad) const {
    if (xst < V || (!packed && xsb < V) || (with_grad && (gst < V || (!packed && gsb < V))))
      return fail(CTC_AMD_EINVAL, "%sstrides smaller than a row of V=%d elements (logits %lld/%lld, grad %lld/%lld)", packed ? "row " : "", V,
                  (long long)xsb, (long long)xst, (long long)gsb, (long long)gst);
    return CTC_AMD_OK;
  }
  Problem applied(Problem p) const {
    p.xsb = xsb; p.xst = xst; p.xdtype = xdtype; p.gsb = gsb; p.gst = gst; p.gdtype = gdtype;
    if (packed) p.row0 = reinterpret_cast<const long long *>(row0);
    return p;
  }
};

// What every producer-format entry point does first, in this order: the common arguments, the element types, B == 0 (CTC_AMD_OK
// and nothing further), a packed batch's row offsets, the strides.  `go`: the call goes on, with `p`; otherwise `rc` is its answer.
struct Prelude { bool go; int rc; Problem p; };
Prelude prelude(const Common &c, const Format &f, bool with_grad, int max_u = MAX_U) {
  if (int rc = check_common(c, max_u)) return {false, rc, {}};
  if (int rc = f.check_dtypes()) return {false, rc, {}};
  if (c.B == 0) return {false, CTC_AMD_OK, {}};
  if (f.packed && !f.row0) return {false, fail(CTC_AMD_EINVAL, "null row_offsets pointer"), {}};
  if (int rc = f.check_strides(c.V, with_grad)) return {false, rc, {}};
  return {true, CTC_AMD_OK, f.applied(make_problem(c))};
}

// ---- checks that several entry points make ----

// everything that stages a token row in LDS; `of_what` ends the message (" of the alignment"; nothing in the size queries)
int check_vocab(int V, const char *of_what = "") {
  if (V > MAX_V_GRAD) return fail(CTC_AMD_EINVAL, "V=%d exceeds the supported maximum %d%s", V, MAX_V_GRAD, of_what);
  return CTC_AMD_OK;
}

// the alignments behind the prelude: the two outputs that must exist, then the vocabulary limit
int check_alignment(const float *score, const int32_t *tokens, int T, int V) {
  if (!score || (T > 0 && !tokens)) return fail(CTC_AMD_EINVAL, "null score / tokens pointer");
  return check_vocab(V, " of the alignment");
}

// the row stages run one workgroup per `rows_per_group` (4 or 16) of the B * T rows
int check_row_grid(int B, int T, int rows_per_group) {
  if (((long long)B * T + rows_per_group - 1) / rows_per_group > 0x7fffffffLL)
    return fail(CTC_AMD_EINVAL, "B * T = %lld rows exceed the launch grid", (long long)B * T);
  return CTC_AMD_OK;
}

int check_wildcard_weight(float w) {
  if (!(w <= 0.f) || w < -3.402823466e38f) return fail(CTC_AMD_EINVAL, "wildcard_log_weight must be finite and <= 0, got %g", (double)w);
  return CTC_AMD_OK;
}

// what the wildcard loss and the entries built on it take behind the prelude; the row stage runs only for a gradient
int check_wildcard_loss(float w, const float *loss, int B, int T, int V, bool row_stage) {
  if (int rc = check_wildcard_weight(w)) return rc;
  if (!loss) return fail(CTC_AMD_EINVAL, "null loss pointer");
  if (int rc = check_vocab(V, " of the wildcard loss")) return rc;
  return row_stage ? check_row_grid(B, T, 4) : CTC_AMD_OK;
}

// the frame windows of the windowed entry points: [B][window_stride] int32 with (first, last) of U label positions per utterance.
// A null pointer is the unwindowed call, whatever the stride says.
int check_window(const int32_t *frame_window, int window_stride, int U) {
  if (frame_window && (long long)window_stride < 2LL * U)
    return fail(CTC_AMD_EINVAL, "window_stride=%d is smaller than 2 * U = %lld", window_stride, 2LL * U);
  return CTC_AMD_OK;
}

// the answer to a long-form plan function that refused
int bad_tiling(int frames_per_tile, int B, int T, int U) {
  return fail(CTC_AMD_EINVAL, "frames_per_tile=%d is neither 0 nor a positive multiple of %d, or B=%d is too large for T=%d U=%d",
              frames_per_tile, CTC_AMD_LONG_FRAMES_MULTIPLE, B, T, U);
}

// A null workspace: refused even where no byte is needed, or taken where none is.  Which of the two an entry point has is part of
// its contract.
enum class NullWs { Refused, TakenIfUnneeded };
int check_workspace(const void *ws, size_t bytes, size_t need, NullWs rule) {
  if (bytes < need || (!ws && (rule == NullWs::Refused || need > 0)))
    return fail(CTC_AMD_EWORKSPACE, "workspace too small: %zu < %zu", bytes, need);
  return CTC_AMD_OK;
}

// every size query looks at its result pointer first
int check_out_bytes(const size_t *out_bytes) { return out_bytes ? CTC_AMD_OK : fail(CTC_AMD_EINVAL, "out_bytes is null"); }

// ... and those that take a lattice shape then at the shape
int check_query_shape(int kind, int B, int T, int V, int U, const size_t *out_bytes, int max_u = MAX_U) {
  if (int rc = check_out_bytes(out_bytes)) return rc;
  if (!shape_ok(kind, B, T, V, U, max_u)) return fail(CTC_AMD_EINVAL, "bad kind or shape: kind=%d B=%d T=%d V=%d U=%d", kind, B, T, V, U);
  return CTC_AMD_OK;
}

// ... and then the vocabulary limit
int check_query(int kind, int B, int T, int V, int U, const size_t *out_bytes, int max_u = MAX_U) {
  if (int rc = check_query_shape(kind, B, T, V, U, out_bytes, max_u)) return rc;
  return check_vocab(V);
}

// a long-form size query: make_plan(&plan) is the entry point's plan function on the query's arguments
template <class Plan, class MakePlan>
int long_query(int kind, int B, int T, int V, int U, int frames_per_tile, size_t *out_bytes, MakePlan make_plan) {
  if (int rc = check_query(kind, B, T, V, U, out_bytes, CTC_AMD_LONG_MAX_U)) return rc;
  Plan plan;
  if (!make_plan(&plan)) return bad_tiling(frames_per_tile, B, T, U);
  *out_bytes = plan.total;
  return CTC_AMD_OK;
}

// what ctc_amd_beam_search and its size query take beyond a shape
int check_beam(int V, int beam_width, int top_k) {
  if (int rc = check_vocab(V, " of the beam search")) return rc;
  if (beam_width < 1 || beam_width > CTC_AMD_BEAM_MAX_WIDTH) return fail(CTC_AMD_EINVAL, "beam_width %d outside [1, %d]", beam_width, CTC_AMD_BEAM_MAX_WIDTH);
  if (top_k < 1 || top_k > CTC_AMD_BEAM_MAX_TOP_K) return fail(CTC_AMD_EINVAL, "top_k %d outside [1, %d]", top_k, CTC_AMD_BEAM_MAX_TOP_K);
  return CTC_AMD_OK;
}

// what the N-best entry points (max_n = CTC_AMD_NBEST_MAX) and the prefix scorer's (CTC_AMD_PREFIX_MAX) take beyond a shape
int check_hypotheses(int B, int V, int N, int max_n, const char *of_what) {
  if (int rc = check_vocab(V, of_what)) return rc;
  if (N < 1 || N > max_n) return fail(CTC_AMD_EINVAL, "N %d outside [1, %d]", N, max_n);
  if ((long long)B * N > 0x7fffffffLL) return fail(CTC_AMD_EINVAL, "B * N = %lld hypotheses exceed 2^31", (long long)B * N);
  return CTC_AMD_OK;
}
int check_nbest(int B, int V, int N) { return check_hypotheses(B, V, N, CTC_AMD_NBEST_MAX, " of the N-best loss"); }
int check_prefix(int B, int V, int N) { return check_hypotheses(B, V, N, CTC_AMD_PREFIX_MAX, " of the prefix scorer"); }

// what the two step calls of the prefix scorer share behind the prelude; only logits need the row statistics
int check_prefix_step(const Problem &p, int N, const void *rows, size_t rows_bytes) {
  if (int rc = check_prefix(p.B, p.V, N)) return rc;
  if (p.wrt == CTC_AMD_WRT_LOGITS && p.T > 0) {
    if (!rows) return fail(CTC_AMD_EINVAL, "null rows pointer (ctc_amd_prefix_rows fills it once per logits tensor)");
    const size_t need = ctc::prefix_rows_bytes(p.B, p.T);
    if (rows_bytes < need) return fail(CTC_AMD_EWORKSPACE, "rows buffer too small: %zu < %zu", rows_bytes, need);
  }
  return CTC_AMD_OK;
}

// The edit-distance entry points and their size queries (max_r: CTC_AMD_MAX_U, or CTC_AMD_LONG_MAX_U for the tiled counts): the
// sizes, which the compute calls check before B == 0, and the pairs, which they check behind it.
int check_edit_sizes(int B, int R, int max_r) {
  if (B < 0 || R < 0) return fail(CTC_AMD_EINVAL, "negative size: B=%d R=%d", B, R);
  if (R > max_r) return fail(CTC_AMD_EINVAL, "R=%d exceeds the supported maximum %d", R, max_r);
  return CTC_AMD_OK;
}
int check_edit_pairs(int B, int N) {
  if (N < 1) return fail(CTC_AMD_EINVAL, "N %d below 1", N);
  if ((long long)B * N > 0x7fffffffLL) return fail(CTC_AMD_EINVAL, "B * N = %lld pairs exceed 2^31", (long long)B * N);
  return CTC_AMD_OK;
}
int check_edit_strides(int hyp_stride, int ref_stride) {
  if (hyp_stride < 0 || ref_stride < 0) return fail(CTC_AMD_EINVAL, "negative stride: hyp_stride=%d ref_stride=%d", hyp_stride, ref_stride);
  return CTC_AMD_OK;
}

static_assert(ctc::EDIT_LONG_MAX_R == CTC_AMD_LONG_MAX_U && ctc::EDIT_LONG_MAX_STRIDE == CTC_AMD_EDIT_COUNTS_MAX_STRIDE &&
              ctc::EDIT_LONG_ROWS_MULTIPLE == CTC_AMD_EDIT_COUNTS_ROWS_MULTIPLE, "include/ctc_amd.h and ctc_edit_long_plan.h disagree");

// the tiling of ctc_amd_edit_counts and its size query, and the plan of a valid one (the size query has no ref_stride: only here
// can its hyp_stride be found negative)
int check_edit_counts_tiling(int B, int N, int R, int hyp_stride, int rows_per_tile, ctc::EditCountsPlan *plan) {
  if (hyp_stride < 0) return fail(CTC_AMD_EINVAL, "negative stride: hyp_stride=%d", hyp_stride);
  if (hyp_stride > CTC_AMD_EDIT_COUNTS_MAX_STRIDE)
    return fail(CTC_AMD_EINVAL, "hyp_stride=%d exceeds the supported maximum %d", hyp_stride, CTC_AMD_EDIT_COUNTS_MAX_STRIDE);
  if (rows_per_tile < 0 || rows_per_tile % CTC_AMD_EDIT_COUNTS_ROWS_MULTIPLE != 0)
    return fail(CTC_AMD_EINVAL, "rows_per_tile=%d is neither 0 nor a positive multiple of %d", rows_per_tile, CTC_AMD_EDIT_COUNTS_ROWS_MULTIPLE);
  if (!ctc::edit_counts_plan(B, N, R, hyp_stride, rows_per_tile, plan))
    return fail(CTC_AMD_EINVAL, "B * N = %lld pairs are too many for the launch grid at R=%d hyp_stride=%d rows_per_tile=%d", (long long)B * N,
                R, hyp_stride, rows_per_tile);
  return CTC_AMD_OK;
}

// ---- tier selection ----

// The loss + gradient pipelines, best last.  Their names cross the ABI in ctc_amd_pipeline_name and ctc_amd_debug_override only.
enum class Tier {
  V1,      // three kernels, emit -> scan -> grad (ctc_kernels.hip): every shape and format
  Fused5,  // one launch, checkpoint + recompute in the log domain (ctc_fused5.hip)
  Fused6,  // the same decomposition in the linear domain (ctc_fused6.hip); utterances beyond its number format are flagged and
           // redone with the log-domain roles inside the same launch
#ifdef CTC_WIDE_EXPERIMENT
  Wide,    // experiments/wide/ only: the three stages of v1 beside each other in one persistent launch, V > 1024, with a gradient
#endif
};

const char *tier_name(Tier t) {
  switch (t) {
    case Tier::Fused5: return "fused5";
    case Tier::Fused6: return "fused6";
#ifdef CTC_WIDE_EXPERIMENT
    case Tier::Wide: return "wide";
#endif
    default: return "v1";
  }
}

// diagnostic overrides (ctc_amd_debug_override): process-wide, written only by tests / benchmarks between calls
Tier g_tier_cap = Tier::Fused6;  // the best tier a call may select (the parity tests run all of them); Wide: that tier or v1
int g_force_hvp_v1 = 0;          // 1 = the log-domain Hessian-vector pipeline also where the fused kernel applies
int g_hvp_diag = 0;              // timing diagnostics of the fused kernel (ctc_hvp_fused.hip `mode`; results are then meaningless)

// What both fused tiers (the same instantiations in ctc_fused5.hip and ctc_fused6.hip) take, term by term:
//   * the gradient with respect to logits, of a non-empty batch with frames;
//   * up to 512 label positions (eight per lane, NL <= 8), with vocabularies up to 512 tokens; up to 128 positions
//     (NL <= 2) with vocabularies up to 1024 -- the LDS budget of the launch tables at the end of the two units;
//   * logits and gradient both float32 or both bfloat16 (float16: three kernels), in a strided batch (packed: three kernels);
//   * float32 in any V, stride and alignment (the element-wise instantiation takes what the 16-byte ones cannot);
//     bfloat16 only with 8-byte aligned rows: V and the four strides multiples of 4, base pointers 8-byte aligned.
bool fused_eligible(const Problem &p) {
  const int NL = ctc::nl_for(p.U);
  return p.wrt == 0 && (p.V <= 512 || (p.V <= 1024 && NL <= 2)) && NL <= 8 && p.B > 0 && p.T > 0 && p.xdtype == p.gdtype &&
         p.xdtype <= 1 && p.row0 == nullptr &&
         (p.xdtype == 0 || (((p.V | p.xsb | p.xst | p.gsb | p.gst) & 3) == 0 && (p.align_bits & 7) == 0));
}

// The best tier the override allows and the call is eligible for; nothing here reads the environment.
// (want_grad: with grad == NULL the fused tiers stop at the meeting point of their two chains; only the parked wide tier declines.)
Tier select_tier(const Problem &p, [[maybe_unused]] bool want_grad) {
#ifdef CTC_WIDE_EXPERIMENT
  if (g_tier_cap == Tier::Wide)
    return want_grad && ctc::wide_eligible(p, ctc::make_layout(p.kind, p.B, p.T, p.U, 0)) ? Tier::Wide : Tier::V1;
#endif
  return g_tier_cap != Tier::V1 && fused_eligible(p) ? g_tier_cap : Tier::V1;
}

// The fused tiers keep one checkpoint row per block and 8 bytes of statistics per frame: their layout is the compact one
// (ctc_common.h Layout::ck_blk); every other pipeline needs full lattice rows.
Layout layout_for(const Problem &p, Tier t) {
  const bool compact = t == Tier::Fused5 || t == Tier::Fused6;
  return ctc::make_layout(p.kind, p.B, p.T, p.U, 0, compact ? ctc::fused_blk(ctc::nl_for(p.U), p.V) : 0);
}

// one translation unit per (tier, lattice kind, label positions per lane): [Fused6?][kind][log2 NL]
ctc::FusedEntry *const fused_entry[2][2][4] = {
    {{ctc::run_fused5_classic_nl1, ctc::run_fused5_classic_nl2, ctc::run_fused5_classic_nl4, ctc::run_fused5_classic_nl8},
     {ctc::run_fused5_simplified_nl1, ctc::run_fused5_simplified_nl2, ctc::run_fused5_simplified_nl4, ctc::run_fused5_simplified_nl8}},
    {{ctc::run_fused6_classic_nl1, ctc::run_fused6_classic_nl2, ctc::run_fused6_classic_nl4, ctc::run_fused6_classic_nl8},
     {ctc::run_fused6_simplified_nl1, ctc::run_fused6_simplified_nl2, ctc::run_fused6_simplified_nl4, ctc::run_fused6_simplified_nl8}}};

hipError_t run_fused(Tier t, const Problem &p, const Layout &L, char *ws, float *loss, const float *d_loss, float *grad, hipStream_t st) {
  const int lg = L.NL == 1 ? 0 : L.NL == 2 ? 1 : L.NL == 4 ? 2 : L.NL == 8 ? 3 : -1;
  if (lg < 0) return hipErrorInvalidValue;
  return fused_entry[t == Tier::Fused6][p.kind][lg](p, L, ws, loss, d_loss, grad, st);
}

// ---- shared bodies ----

int add_loss_sum(const float *loss, int B, long long *sum2, long long *zero_next, hipStream_t st) {
  CTC_TRY(ctc::run_sum_loss_fixed(loss, B, sum2, zero_next, st), "loss sum launch");
  return CTC_AMD_OK;
}

int loss_grad_impl(Problem p, float *loss, void *grad, const float *d_loss, void *workspace, size_t workspace_bytes, void *stream) {
  if (!loss) return fail(CTC_AMD_EINVAL, "null loss pointer");
  if (int rc = grad ? check_vocab(p.V, " for the gradient") : CTC_AMD_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float *gradf = static_cast<float *>(grad);  // element-typed inside the kernels (Problem::gdtype)
  p.align_bits = low_bits(p.logits, grad);
  const Tier tier = select_tier(p, grad != nullptr);
  const Layout L = layout_for(p, tier);
  if (!workspace || workspace_bytes < L.total)
    return fail(CTC_AMD_EWORKSPACE, "workspace too small for pipeline %s: %zu < %zu", tier_name(tier), workspace_bytes, L.total);
  char *ws = static_cast<char *>(workspace);
  switch (tier) {
    case Tier::Fused5:
    case Tier::Fused6:
      CTC_TRY(run_fused(tier, p, L, ws, loss, d_loss, gradf, st), tier_name(tier));
      break;
#ifdef CTC_WIDE_EXPERIMENT
    case Tier::Wide:
      CTC_TRY(ctc::run_wide(p, L, ws, loss, d_loss, gradf, st), "wide launch");
      break;
#endif
    case Tier::V1:
      CTC_TRY(ctc::run_emit_scan(p, L, ws, loss, grad ? 2 : 1, st), "emit/scan launch");
      if (grad) CTC_TRY(ctc::run_grad(p, L, ws, d_loss, gradf, st), "grad launch");
      break;
  }
  if (p.sum_out && tier != Tier::Fused6) return add_loss_sum(loss, p.B, p.sum_out, p.sum_zero, st);  // (fused6 adds inside its launch)
  return CTC_AMD_OK;
}

// The log-domain entry points (alpha/beta, log posterior, Hessian, HVP) read contiguous float32 logits and full lattice rows:
// layout with `extra` bytes behind them, workspace check, Problem.
struct LogDomain { Layout L; Problem p; char *ws; hipStream_t st; };
int log_domain_setup(const Common &c, size_t extra, void *workspace, size_t workspace_bytes, void *stream, LogDomain &d) {
  d.L = ctc::make_layout(c.kind, c.B, c.T, c.U, extra);
  if (int rc = check_workspace(workspace, workspace_bytes, d.L.total, NullWs::Refused)) return rc;
  d.p = make_problem(c);
  d.ws = static_cast<char *>(workspace);
  d.st = static_cast<hipStream_t>(stream);
  return CTC_AMD_OK;
}

static_assert(ctc::LONG_LOSS_WILDCARD == CTC_AMD_WILDCARD, "the tiled loss kernel's wildcard label is the ABI's");
static_assert(ctc::LONG_LOSS_OPTIONAL == CTC_AMD_OPTIONAL_WILDCARD, "the tiled loss kernel's optional wildcard label is the ABI's");

// ctc_amd_long_wildcard_loss_grad and its checkpointed twin, which differ in the plan function alone (long_loss_ckpt_plan refuses
// what long_loss_plan refuses, and is long_loss_plan without a gradient).  The window is looked at behind every check of the unwindowed
// call but the workspace's.  optional_wildcards (ctc_amd_long_optional_wildcard_loss_grad / _grad_ckpt, which have no window): the
// same checks, the plan with the two further column buffers.
using LongLossPlanFn = bool(int, int, int, int, int, int, ctc::LongLossPlan *, int);
int long_wildcard_loss_grad_impl(LongLossPlanFn *plan_fn, bool optional_wildcards, const Common &c, const Format &f,
                                 const int32_t *frame_window, int window_stride, float wildcard_log_weight, int frames_per_tile, const float *d_loss, float *loss, void *grad,
                                 void *workspace, size_t workspace_bytes, void *stream) {
  const Prelude pre = prelude(c, f, grad != nullptr, CTC_AMD_LONG_MAX_U);
  if (!pre.go) return pre.rc;
  if (int rc = check_wildcard_loss(wildcard_log_weight, loss, c.B, c.T, c.V, grad != nullptr)) return rc;
  ctc::LongLossPlan plan;
  if (!plan_fn(c.kind, c.B, c.T, c.U, frames_per_tile, grad != nullptr, &plan, optional_wildcards ? 1 : 0))
    return bad_tiling(frames_per_tile, c.B, c.T, c.U);
  if (int rc = check_window(frame_window, window_stride, c.U)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, plan.total, NullWs::Refused)) return rc;
  CTC_TRY(ctc::run_loss_long(pre.p, plan, wildcard_log_weight, d_loss, loss, grad, static_cast<char *>(workspace),
                             static_cast<hipStream_t>(stream), frame_window, window_stride, optional_wildcards),
          "long wildcard loss launch");
  return CTC_AMD_OK;
}

}  // namespace

extern "C" {

int ctc_amd_abi_version(void) { return CTC_AMD_ABI_VERSION; }

const char *ctc_amd_last_error(void) { return g_err; }

int ctc_amd_debug_override(const char *key, const char *value) {
  if (!key || !value) return fail(CTC_AMD_EINVAL, "null key/value");
  if (!strcmp(key, "pipeline")) {
    if (!strcmp(value, "")) g_tier_cap = Tier::Fused6;
    else if (!strcmp(value, "v1")) g_tier_cap = Tier::V1;
    else if (!strcmp(value, "fused5")) g_tier_cap = Tier::Fused5;
#ifdef CTC_WIDE_EXPERIMENT
    else if (!strcmp(value, "wide")) g_tier_cap = Tier::Wide;
#endif
    else return fail(CTC_AMD_EINVAL, "pipeline override must be \"\", \"v1\" or \"fused5\", got \"%s\"", value);
    return CTC_AMD_OK;
  }
  if (!strcmp(key, "hessian")) {
    if (strcmp(value, "") && strcmp(value, "slab")) return fail(CTC_AMD_EINVAL, "hessian override must be \"\" or \"slab\", got \"%s\"", value);
    ctc::g_force_hessian_slab = !strcmp(value, "slab");
    return CTC_AMD_OK;
  }
  if (!strcmp(key, "hvp")) {
    int dm = 0;
    if (!strncmp(value, "diag", 4) && sscanf(value + 4, "%d", &dm) == 1 && dm >= 0 && dm <= 31) {  // timing diagnostics (scripts/hvp_time.py)
      g_hvp_diag = dm;
      g_force_hvp_v1 = 0;
      return CTC_AMD_OK;
    }
    if (strcmp(value, "") && strcmp(value, "v1")) return fail(CTC_AMD_EINVAL, "hvp override must be \"\" or \"v1\", got \"%s\"", value);
    g_force_hvp_v1 = !strcmp(value, "v1");
    g_hvp_diag = 0;
    return CTC_AMD_OK;
  }
#ifdef CTC_WIDE_EXPERIMENT
  if (!strcmp(key, "wide")) {  // timing diagnostics (experiments/wide/wide_time.py): "" or "diag<number 0..511>"
    int v = 0;
    if (strcmp(value, "") && (sscanf(value, "diag%d", &v) != 1 || v < 0 || v > 511)) return fail(CTC_AMD_EINVAL, "wide override must be \"\" or \"diag0\"..\"diag511\", got \"%s\"", value);
    ctc::g_wide_diag = v;
    return CTC_AMD_OK;
  }
#endif
  return fail(CTC_AMD_EINVAL, "unknown override key \"%s\"", key);
}

const char *ctc_amd_pipeline_name(int kind, int wrt, int B, int T, int V, int U, int want_grad) {
  if (!shape_ok(kind, B, T, V, U)) return "invalid";
  return tier_name(select_tier(shape_problem(kind, wrt, B, T, V, U), want_grad != 0));
}

int ctc_amd_debug_flags_offset(int kind, int B, int T, int V, int U, size_t *out_offset) {
  if (!out_offset) return fail(CTC_AMD_EINVAL, "out_offset is null");
  if (!shape_ok(kind, B, T, V, U)) return fail(CTC_AMD_EINVAL, "bad shape");
  const Problem p = shape_problem(kind, CTC_AMD_WRT_LOGITS, B, T, V, U);
  const Tier tier = select_tier(p, true);
  if (tier != Tier::Fused6) return fail(CTC_AMD_EINVAL, "these shapes run the %s pipeline, which keeps no flags", tier_name(tier));
  *out_offset = layout_for(p, tier).off_flags;
  return CTC_AMD_OK;
}

int ctc_amd_debug_hvp_flags_offset(int kind, int B, int T, int V, int U, size_t *out_offset) {
  if (!out_offset) return fail(CTC_AMD_EINVAL, "out_offset is null");
  if (!shape_ok(kind, B, T, V, U)) return fail(CTC_AMD_EINVAL, "bad shape");
  if (!ctc::hvp_fused_shape(CTC_AMD_WRT_LOGITS, B, T, V, U)) return fail(CTC_AMD_EINVAL, "these shapes run the log-domain Hessian-vector pipeline, which keeps no flags");
  *out_offset = ctc::make_layout(kind, B, T, U, 0).off_extra + ctc::hvp_fused_flags_offset(kind, B, T, U);
  return CTC_AMD_OK;
}

int ctc_amd_reduce_loss(const float *loss, int B, float *out2, void *stream) {
  if (B < 0 || !out2 || (B > 0 && !loss)) return fail(CTC_AMD_EINVAL, "bad arguments");
  CTC_TRY(ctc::run_reduce_loss(loss, B, out2, static_cast<hipStream_t>(stream)), "reduce launch");
  return CTC_AMD_OK;
}

int ctc_amd_probe_copy(void *dst, const void *src, size_t bytes, void *stream) {
  if (!dst || !src || (bytes & 15) || low_bits(dst, src) != 0) return fail(CTC_AMD_EINVAL, "probe copy needs 16-byte aligned pointers and size");
  CTC_TRY(ctc::run_probe_copy(dst, src, bytes, static_cast<hipStream_t>(stream)), "probe copy launch");
  return CTC_AMD_OK;
}

int ctc_amd_probe_spin(int threads, int lds_bytes, float microseconds, void *stream) {
  if (threads < 64 || threads > 1024 || (threads & 63) || lds_bytes < 0 || lds_bytes > 65536 || !(microseconds >= 0.f) || microseconds > 1000.f)
    return fail(CTC_AMD_EINVAL, "probe spin: threads in 64..1024 (multiple of 64), lds_bytes <= 65536, microseconds <= 1000");
  CTC_TRY(ctc::run_probe_spin(threads, lds_bytes, microseconds, static_cast<hipStream_t>(stream)), "probe spin launch");
  return CTC_AMD_OK;
}

int ctc_amd_check_labels(const int32_t *labels, int label_stride, const int32_t *label_length, int blank_index, int B, int V,
                         int U, void *stream) {
  if (B < 0 || V <= 0 || U < 0 || label_stride < 0) return fail(CTC_AMD_EINVAL, "negative size");
  if (B == 0 || label_stride == 0) return CTC_AMD_OK;
  if (!labels || !label_length) return fail(CTC_AMD_EINVAL, "null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  int *bad = nullptr;
  CTC_TRY(hipMallocAsync(reinterpret_cast<void **>(&bad), sizeof(int), st), "hipMallocAsync");
  hipError_t e = ctc::run_check_labels(labels, label_stride, label_length, blank_index, B, V, U, bad, st);
  int host = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&host, bad, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  hipFreeAsync(bad, st);
  if (e != hipSuccess) return hip_fail(e, "label check");
  if (host != 0) return fail(CTC_AMD_ELABEL, "%d label(s) inside label_length are outside [0, %d) or equal to blank_index %d", host, V, blank_index);
  return CTC_AMD_OK;
}

int ctc_amd_workspace_bytes(int what, int kind, int B, int T, int V, int U, size_t *out_bytes) {
  if (int rc = check_query_shape(kind, B, T, V, U, out_bytes)) return rc;  // (no vocabulary limit: the loss alone has none)
  size_t extra = 0;
  if (what == CTC_AMD_WS_LOSS_GRAD_LOGITS) {
    // the pipeline a float32 / aligned bfloat16 logits call of this shape selects; its own (smaller) layout when that is a fused tier
    const Problem p = shape_problem(kind, CTC_AMD_WRT_LOGITS, B, T, V, U);
    *out_bytes = layout_for(p, select_tier(p, true)).total;
    return CTC_AMD_OK;
  }
  if (what == CTC_AMD_WS_HESSIAN) extra = ctc::hessian_extra_bytes(kind, B, T, V, U);
  else if (what == CTC_AMD_WS_HVP) extra = ctc::hvp_extra_bytes(kind, B, T, V, U);
  else if (what != CTC_AMD_WS_LOSS_GRAD && what != CTC_AMD_WS_ALPHA_BETA) return fail(CTC_AMD_EINVAL, "bad workspace selector %d", what);
  *out_bytes = ctc::make_layout(kind, B, T, U, extra).total;
  return CTC_AMD_OK;
}

int ctc_amd_loss_grad(int kind, int wrt, const float *logits, const int32_t *labels, int label_stride,
                      const int32_t *label_length, const int32_t *logit_length, int blank_index, int B, int T, int V,
                      int U, float *loss, float *grad, const float *d_loss, void *workspace, size_t workspace_bytes,
                      void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  if (int rc = check_common(c)) return rc;
  if (B == 0) return CTC_AMD_OK;
  return loss_grad_impl(make_problem(c), loss, grad, d_loss, workspace, workspace_bytes, stream);
}

// Every entry point from here on that takes a producer format begins with prelude() and goes on with what only it takes; the
// order of those checks is part of the contract (tests/golden/cabi_fault_matrix.json).  Two historical exceptions are part of it
// too and make the prelude's steps by hand: ctc_amd_loss_grad_sum looks at sum2 before the element types and at its strides before
// B == 0 (an empty batch still clears the next step's buffer), ctc_amd_grad_resume at its gradient pointer before B == 0.

int ctc_amd_loss_grad_ex(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                         int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                         const int32_t *logit_length, int blank_index, int B, int T, int V, int U, float *loss, void *grad,
                         int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t, const float *d_loss, void *workspace,
                         size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, logits_stride_b, logits_stride_t, grad_dtype, grad_stride_b, grad_stride_t};
  const Prelude pre = prelude(c, f, grad != nullptr);
  if (!pre.go) return pre.rc;
  return loss_grad_impl(pre.p, loss, grad, d_loss, workspace, workspace_bytes, stream);
}

int ctc_amd_loss_grad_packed(int kind, int wrt, const void *logits, int logits_dtype, const int64_t *row_offsets, int64_t row_stride,
                             const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                             int blank_index, int B, int T, int V, int U, float *loss, void *grad, int grad_dtype,
                             int64_t grad_row_stride, const float *d_loss, void *workspace, size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, 0, row_stride, grad_dtype, 0, grad ? grad_row_stride : V, true, row_offsets};
  const Prelude pre = prelude(c, f, grad != nullptr);
  if (!pre.go) return pre.rc;
  return loss_grad_impl(pre.p, loss, grad, d_loss, workspace, workspace_bytes, stream);
}

int ctc_amd_loss_grad_sum(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                          int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                          const int32_t *logit_length, int blank_index, int B, int T, int V, int U, float *loss, void *grad,
                          int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t, const float *d_loss, long long *sum2,
                          long long *zero_next, void *workspace, size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, logits_stride_b, logits_stride_t, grad_dtype, grad_stride_b, grad_stride_t};
  if (int rc = check_common(c)) return rc;
  if (!sum2) return fail(CTC_AMD_EINVAL, "null sum2 pointer");
  if (int rc = f.check_dtypes()) return rc;
  if (int rc = f.check_strides(V, grad != nullptr)) return rc;
  if (B == 0)  // nothing to add; the next step's buffer still has to be cleared
    return zero_next ? add_loss_sum(loss, 0, sum2, zero_next, static_cast<hipStream_t>(stream)) : CTC_AMD_OK;
  Problem p = f.applied(make_problem(c));
  p.sum_out = sum2; p.sum_zero = zero_next;
  return loss_grad_impl(p, loss, grad, d_loss, workspace, workspace_bytes, stream);
}

int ctc_amd_loss_forward(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                         int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                         const int32_t *logit_length, int blank_index, int B, int T, int V, int U, float *loss, void *workspace,
                         size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  // (no gradient in this half: the pipeline is chosen as for a gradient in the logits' own format, which is what the front ends ask
  // ctc_amd_grad_resume for)
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false);
  if (!pre.go) return pre.rc;
  Problem p = pre.p;
  // (Problem::resume: 0 = a call of its own, 1 = second half of a pair, 2 = first half of a pair -- the linear-domain kernel then
  // honours its conservative loss-only signs for binding alignments only, ctc_fused6.hip; other pipelines do not look at it)
  p.resume = 2;
  return loss_grad_impl(p, loss, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int ctc_amd_grad_resume(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                        int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                        const int32_t *logit_length, int blank_index, int B, int T, int V, int U, float *loss, void *grad,
                        int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t, const float *d_loss, void *workspace,
                        size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, logits_stride_b, logits_stride_t, grad_dtype, grad_stride_b, grad_stride_t};
  if (int rc = check_common(c)) return rc;
  if (int rc = f.check_dtypes()) return rc;
  if (!grad) return fail(CTC_AMD_EINVAL, "null grad pointer");
  if (B == 0) return CTC_AMD_OK;
  if (int rc = f.check_strides(V, true)) return rc;
  Problem p = f.applied(make_problem(c));
  // only the linear-domain fused kernel keeps what the second half needs; every other pipeline computes loss and gradient anew
  // (eligibility is decided on the same alignment bits the launch will see)
  p.align_bits = low_bits(p.logits, grad);
  if (select_tier(p, true) == Tier::Fused6) p.resume = 1;
  return loss_grad_impl(p, loss, grad, d_loss, workspace, workspace_bytes, stream);
}

int ctc_amd_alpha_beta(int kind, int wrt, const float *logits, const int32_t *labels, int label_stride,
                       const int32_t *label_length, const int32_t *logit_length, int blank_index, int B, int T, int V,
                       int U, float *loss, float *alpha, float *beta, void *workspace, size_t workspace_bytes,
                       void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  if (int rc = check_common(c)) return rc;
  if (B == 0) return CTC_AMD_OK;
  if (!loss || !alpha || !beta) return fail(CTC_AMD_EINVAL, "null output pointer");
  LogDomain d;
  if (int rc = log_domain_setup(c, 0, workspace, workspace_bytes, stream, d)) return rc;
  const auto &[L, p, ws, st] = d;
  CTC_TRY(ctc::run_emit_scan(p, L, ws, loss, 2, st), "emit/scan launch");
  CTC_TRY(ctc::run_convert(p, L, ws, alpha, beta, st), "convert launch");
  return CTC_AMD_OK;
}

int ctc_amd_log_posterior(int kind, int wrt, const float *logits, const int32_t *labels, int label_stride,
                          const int32_t *label_length, const int32_t *logit_length, int blank_index, int B, int T, int V,
                          int U, float *loss, float *lg, void *workspace, size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  if (int rc = check_common(c)) return rc;
  if (B == 0) return CTC_AMD_OK;
  if (!loss || (T > 0 && !lg)) return fail(CTC_AMD_EINVAL, "null output pointer");
  if (V > 8192) return fail(CTC_AMD_EINVAL, "V=%d exceeds the supported maximum 8192 of ctc_amd_log_posterior", V);
  LogDomain d;
  if (int rc = log_domain_setup(c, 0, workspace, workspace_bytes, stream, d)) return rc;
  const auto &[L, p, ws, st] = d;
  CTC_TRY(ctc::run_emit_scan(p, L, ws, loss, 2, st), "emit/scan launch");
  CTC_TRY(ctc::run_log_posterior(p, L, ws, lg, st), "log posterior launch");
  return CTC_AMD_OK;
}

int ctc_amd_hessian(int kind, int wrt, const float *logits, const int32_t *labels, int label_stride,
                    const int32_t *label_length, const int32_t *logit_length, int blank_index, int B, int T, int V,
                    int U, float *loss, float *grad, float *hess, void *workspace, size_t workspace_bytes,
                    void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  if (int rc = check_common(c)) return rc;
  if (B == 0) return CTC_AMD_OK;
  if (!loss || !hess) return fail(CTC_AMD_EINVAL, "null output pointer");
  if (V > MAX_V_HESS) return fail(CTC_AMD_EINVAL, "V=%d exceeds the supported maximum %d of the Hessian", V, MAX_V_HESS);
  if (low_bits(logits, grad, hess) != 0) return fail(CTC_AMD_EINVAL, "ctc_amd_hessian needs 16-byte aligned logits / grad / hess pointers");
  LogDomain d;
  if (int rc = log_domain_setup(c, ctc::hessian_extra_bytes(kind, B, T, V, U), workspace, workspace_bytes, stream, d)) return rc;
  const auto &[L, p, ws, st] = d;
  CTC_TRY(ctc::run_emit_scan(p, L, ws, loss, 2, st), "emit/scan launch");
  // the Hessian needs the log-probability-space gradient g = -posterior; it lives in the extra workspace region
  float *g_lp = reinterpret_cast<float *>(ws + L.off_extra);
  Problem plp = p;
  plp.wrt = CTC_AMD_WRT_LOGPROBS;
  // grad_kernel only reads emis/alpha/beta/logp; with wrt = LOGPROBS it writes -posterior
  CTC_TRY(ctc::run_grad(plp, L, ws, nullptr, g_lp, st), "posterior launch");
  if (grad) CTC_TRY(ctc::run_grad(p, L, ws, nullptr, grad, st), "grad launch");
  CTC_TRY(ctc::run_hessian(p, L, ws, g_lp, hess, st), "hessian launch");
  return CTC_AMD_OK;
}

int ctc_amd_hvp(int kind, int wrt, const float *logits, const int32_t *labels, int label_stride,
                const int32_t *label_length, const int32_t *logit_length, int blank_index, int B, int T, int V, int U,
                const float *vec, float *loss, float *grad, float *out, void *workspace, size_t workspace_bytes,
                void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  if (int rc = check_common(c)) return rc;
  if (B == 0) return CTC_AMD_OK;
  if (!loss || !out || (T > 0 && !vec)) return fail(CTC_AMD_EINVAL, "null vec/output pointer");
  if (V > MAX_V_HESS) return fail(CTC_AMD_EINVAL, "V=%d exceeds the supported maximum %d of the Hessian-vector product", V, MAX_V_HESS);
  if (low_bits(logits, vec, grad, out) != 0) return fail(CTC_AMD_EINVAL, "ctc_amd_hvp needs 16-byte aligned logits / vec / grad / out pointers");
  LogDomain d;
  if (int rc = log_domain_setup(c, ctc::hvp_extra_bytes(kind, B, T, V, U), workspace, workspace_bytes, stream, d)) return rc;
  const auto &[L, p, ws, st] = d;
  // The fused linear-domain kernel (ctc_hvp_fused.hip) where its instantiations apply: ONE launch; utterances its number format
  // cannot hold are redone by their own workgroup with the log-domain building blocks, inside the same launch.
  if (!grad && !g_force_hvp_v1 && ctc::hvp_fused_shape(wrt, B, T, V, U)) {
    CTC_TRY((kind == 0 ? ctc::run_hvp_fused_classic : ctc::run_hvp_fused_simplified)(p, L, ws, vec, loss, out, g_hvp_diag, st), "fused hvp launch");
    return CTC_AMD_OK;
  }
  CTC_TRY(ctc::run_emit_scan(p, L, ws, loss, 2 | 4, st), "emit/scan launch");  // (+ 4: rows renormalised every step, for the tangent sweep)
  if (grad) CTC_TRY(ctc::run_grad(p, L, ws, nullptr, grad, st), "grad launch");
  CTC_TRY(ctc::run_hvp(p, L, ws, vec, out, st), "hvp launch");
  return CTC_AMD_OK;
}

int ctc_amd_best_path_workspace_bytes(int kind, int B, int T, int V, int U, size_t *out_bytes) {
  if (int rc = check_query(kind, B, T, V, U, out_bytes)) return rc;
  *out_bytes = ctc::align_workspace_bytes(B, T, U);
  return CTC_AMD_OK;
}

int ctc_amd_best_path(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                      const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                      int blank_index, int B, int T, int V, int U, float *score, int32_t *tokens, int32_t *label_index,
                      void *workspace, size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false);
  if (!pre.go) return pre.rc;
  if (int rc = check_alignment(score, tokens, T, V)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, ctc::align_workspace_bytes(B, T, U), NullWs::Refused)) return rc;
  CTC_TRY(ctc::run_align(pre.p, static_cast<char *>(workspace), score, tokens, label_index, static_cast<hipStream_t>(stream)), "alignment launch");
  return CTC_AMD_OK;
}

int ctc_amd_greedy_decode_workspace_bytes(int B, int T, size_t *out_bytes) {
  if (int rc = check_out_bytes(out_bytes)) return rc;
  if (B < 0 || T < 0) return fail(CTC_AMD_EINVAL, "negative size: B=%d T=%d", B, T);
  *out_bytes = ctc::decode_workspace_bytes(B, T);
  return CTC_AMD_OK;
}

// It takes no labels: an empty label tensor stands in for them.  No vocabulary limit: no row is staged in LDS.
int ctc_amd_greedy_decode(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                          const int32_t *logit_length, int blank_index, int B, int T, int V, float *score, int32_t *tokens,
                          int32_t *decoded, int32_t *decoded_length, int32_t *frames, float *label_score, void *workspace,
                          size_t workspace_bytes, void *stream) {
  // (label_length: only its null check applies, and logit_length answers it)
  const Common c{kind, wrt, logits, nullptr, 0, logit_length, logit_length, blank_index, B, T, V, 0};
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false);
  if (!pre.go) return pre.rc;
  if (!score || !decoded_length || (T > 0 && (!tokens || !decoded)))
    return fail(CTC_AMD_EINVAL, "null score / tokens / decoded / decoded_length pointer");
  if (int rc = check_row_grid(B, T, 16)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, ctc::decode_workspace_bytes(B, T), NullWs::TakenIfUnneeded)) return rc;
  CTC_TRY(ctc::run_decode(pre.p, static_cast<char *>(workspace), score, tokens, decoded, decoded_length, frames, label_score,
                          static_cast<hipStream_t>(stream)), "greedy decode launch");
  return CTC_AMD_OK;
}

int ctc_amd_beam_search_workspace_bytes(int B, int T, int V, int beam_width, int top_k, size_t *out_bytes) {
  if (int rc = check_out_bytes(out_bytes)) return rc;
  if (B < 0 || T < 0 || V <= 0) return fail(CTC_AMD_EINVAL, "negative size: B=%d T=%d V=%d", B, T, V);
  if (int rc = check_beam(V, beam_width, top_k)) return rc;
  *out_bytes = ctc::beam_workspace_bytes(B, T, V, beam_width, top_k);
  return CTC_AMD_OK;
}

// No labels, as in ctc_amd_greedy_decode.
int ctc_amd_beam_search(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                        const int32_t *logit_length, int blank_index, int B, int T, int V, int beam_width, int top_k, int nbest,
                        float *score, int32_t *decoded, int32_t *decoded_length, void *workspace, size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, nullptr, 0, logit_length, logit_length, blank_index, B, T, V, 0};
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false);
  if (!pre.go) return pre.rc;
  if (int rc = check_beam(V, beam_width, top_k)) return rc;
  if (nbest < 1 || nbest > beam_width) return fail(CTC_AMD_EINVAL, "nbest %d outside [1, beam_width = %d]", nbest, beam_width);
  if (!score || !decoded_length || (T > 0 && !decoded)) return fail(CTC_AMD_EINVAL, "null score / decoded / decoded_length pointer");
  if (int rc = check_row_grid(B, T, 16)) return rc;
  if ((long long)beam_width * T + 1 > 0x7fffffffLL) return fail(CTC_AMD_EINVAL, "beam_width * T = %lld prefix nodes exceed 2^31", (long long)beam_width * T);
  if (int rc = check_workspace(workspace, workspace_bytes, ctc::beam_workspace_bytes(B, T, V, beam_width, top_k), NullWs::Refused)) return rc;
  CTC_TRY(ctc::run_beam(pre.p, beam_width, top_k, nbest, static_cast<char *>(workspace), score, decoded, decoded_length,
                        static_cast<hipStream_t>(stream)), "beam search launch");
  return CTC_AMD_OK;
}

int ctc_amd_nbest_loss_workspace_bytes(int kind, int B, int T, int V, int U, int N, size_t *out_bytes) {
  if (int rc = check_query_shape(kind, B, T, V, U, out_bytes)) return rc;
  if (int rc = check_nbest(B, V, N)) return rc;
  *out_bytes = ctc::nbest_workspace_bytes(kind, B, T, V, U, N);
  return CTC_AMD_OK;
}

// It needs no workspace today, so a null one passes.
int ctc_amd_nbest_loss(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                       const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                       int blank_index, int B, int T, int V, int U, int N, float *loss, void *workspace, size_t workspace_bytes,
                       void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false);
  if (!pre.go) return pre.rc;
  if (int rc = check_nbest(B, V, N)) return rc;
  if (!loss) return fail(CTC_AMD_EINVAL, "null loss pointer");
  if (int rc = check_workspace(workspace, workspace_bytes, ctc::nbest_workspace_bytes(kind, B, T, V, U, N), NullWs::TakenIfUnneeded)) return rc;
  CTC_TRY(ctc::run_nbest(pre.p, N, loss, static_cast<hipStream_t>(stream)), "N-best loss launch");
  return CTC_AMD_OK;
}

int ctc_amd_nbest_loss_grad_workspace_bytes(int kind, int B, int T, int V, int U, int N, size_t *out_bytes) {
  if (int rc = check_query_shape(kind, B, T, V, U, out_bytes)) return rc;
  if (int rc = check_nbest(B, V, N)) return rc;
  *out_bytes = ctc::nbest_grad_workspace_bytes(kind, B, T, V, U, N);
  return CTC_AMD_OK;
}

int ctc_amd_nbest_loss_grad(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                            const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                            int blank_index, int B, int T, int V, int U, int N, const float *weight, float *loss, void *grad,
                            int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t, void *workspace, size_t workspace_bytes,
                            void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, logits_stride_b, logits_stride_t, grad_dtype, grad_stride_b, grad_stride_t};
  const Prelude pre = prelude(c, f, true);  // (the gradient's strides are looked at before its pointer)
  if (!pre.go) return pre.rc;
  if (int rc = check_nbest(B, V, N)) return rc;
  if (!weight || !loss || !grad) return fail(CTC_AMD_EINVAL, "null weight / loss / grad pointer");
  if (int rc = check_row_grid(B, T, 4)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, ctc::nbest_grad_workspace_bytes(kind, B, T, V, U, N), NullWs::Refused)) return rc;
  CTC_TRY(ctc::run_nbest_grad(pre.p, N, weight, loss, grad, static_cast<char *>(workspace), static_cast<hipStream_t>(stream)),
          "N-best loss gradient launch");
  return CTC_AMD_OK;
}

int ctc_amd_nbest_best_path_workspace_bytes(int kind, int B, int T, int V, int U, int N, size_t *out_bytes) {
  if (int rc = check_query_shape(kind, B, T, V, U, out_bytes)) return rc;
  if (int rc = check_nbest(B, V, N)) return rc;
  *out_bytes = ctc::nbest_align_workspace_bytes(B, T, U, N);
  return CTC_AMD_OK;
}

int ctc_amd_nbest_best_path(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                            const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                            int blank_index, int B, int T, int V, int U, int N, float *score, int32_t *tokens, int32_t *label_index,
                            int32_t *first_frame, int32_t *last_frame, void *workspace, size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false);
  if (!pre.go) return pre.rc;
  if (int rc = check_nbest(B, V, N)) return rc;
  if (!score || (T > 0 && !tokens)) return fail(CTC_AMD_EINVAL, "null score / tokens pointer");
  if (int rc = check_workspace(workspace, workspace_bytes, ctc::nbest_align_workspace_bytes(B, T, U, N), NullWs::TakenIfUnneeded)) return rc;
  CTC_TRY(ctc::run_nbest_align(pre.p, N, static_cast<char *>(workspace), score, tokens, label_index, first_frame, last_frame,
                               static_cast<hipStream_t>(stream)), "N-best alignment launch");
  return CTC_AMD_OK;
}

static_assert(ctc::ALIGN_WILDCARD == CTC_AMD_WILDCARD, "the kernel's wildcard label is the ABI's");

int ctc_amd_wildcard_best_path_workspace_bytes(int kind, int B, int T, int V, int U, size_t *out_bytes) {
  if (int rc = check_query(kind, B, T, V, U, out_bytes)) return rc;
  *out_bytes = ctc::align_wild_workspace_bytes(B, T, U);
  return CTC_AMD_OK;
}

static_assert(ctc::ALIGN_OPTIONAL == CTC_AMD_OPTIONAL_WILDCARD && ctc::ALIGN_OPTIONAL_CLASSIC_MAX_U == CTC_AMD_OPTIONAL_CLASSIC_MAX_U,
              "the alignment kernel's optional wildcard label and its classic limit are the ABI's");

// the one limit of its own that ctc_amd_optional_wildcard_best_path has (behind the counterpart's checks, before the workspace)
static int check_optional_alignment(bool optional_wildcards, int kind, int U) {
  if (optional_wildcards && kind == CTC_AMD_CLASSIC && U > CTC_AMD_OPTIONAL_CLASSIC_MAX_U)
    return fail(CTC_AMD_EINVAL, "U=%d exceeds CTC_AMD_OPTIONAL_CLASSIC_MAX_U=%d of the classic optional-wildcard alignment", U,
                CTC_AMD_OPTIONAL_CLASSIC_MAX_U);
  return CTC_AMD_OK;
}

// One body for ctc_amd_windowed_best_path and ctc_amd_optional_wildcard_best_path (which has no window).
static int wildcard_best_path_call(bool optional_wildcards, int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                   int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                   const int32_t *logit_length, int blank_index, const int32_t *frame_window, int window_stride, int B,
                                   int T, int V, int U, float *score, int32_t *tokens, int32_t *label_index, int32_t *first_frame,
                                   int32_t *last_frame, float *label_score, void *workspace, size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false);
  if (!pre.go) return pre.rc;
  if (int rc = check_alignment(score, tokens, T, V)) return rc;
  if (int rc = check_window(frame_window, window_stride, U)) return rc;
  if (int rc = check_optional_alignment(optional_wildcards, kind, U)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, ctc::align_wild_workspace_bytes(B, T, U), NullWs::Refused)) return rc;
  CTC_TRY(ctc::run_align_wild(pre.p, static_cast<char *>(workspace), score, tokens, label_index, first_frame, last_frame, label_score,
                              static_cast<hipStream_t>(stream), frame_window, window_stride, optional_wildcards),
          "wildcard alignment launch");
  return CTC_AMD_OK;
}

// The four windowed entry points are their counterparts with a frame window; the counterparts are they with none.
int ctc_amd_windowed_best_path(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                               const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                               int blank_index, const int32_t *frame_window, int window_stride, int B, int T, int V, int U, float *score,
                               int32_t *tokens, int32_t *label_index, int32_t *first_frame, int32_t *last_frame, float *label_score,
                               void *workspace, size_t workspace_bytes, void *stream) {
  return wildcard_best_path_call(false, kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride,
                                 label_length, logit_length, blank_index, frame_window, window_stride, B, T, V, U, score, tokens,
                                 label_index, first_frame, last_frame, label_score, workspace, workspace_bytes, stream);
}

// The back-pointer words have room for the two further sources: the counterpart's workspace.
int ctc_amd_optional_wildcard_best_path_workspace_bytes(int kind, int B, int T, int V, int U, size_t *out_bytes) {
  if (int rc = ctc_amd_wildcard_best_path_workspace_bytes(kind, B, T, V, U, out_bytes)) return rc;
  return check_optional_alignment(true, kind, U);
}

int ctc_amd_optional_wildcard_best_path(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                        int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                        const int32_t *logit_length, int blank_index, int B, int T, int V, int U, float *score,
                                        int32_t *tokens, int32_t *label_index, int32_t *first_frame, int32_t *last_frame,
                                        float *label_score, void *workspace, size_t workspace_bytes, void *stream) {
  return wildcard_best_path_call(true, kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride,
                                 label_length, logit_length, blank_index, nullptr, 0, B, T, V, U, score, tokens, label_index, first_frame,
                                 last_frame, label_score, workspace, workspace_bytes, stream);
}

int ctc_amd_wildcard_best_path(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                               const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                               int blank_index, int B, int T, int V, int U, float *score, int32_t *tokens, int32_t *label_index,
                               int32_t *first_frame, int32_t *last_frame, float *label_score, void *workspace, size_t workspace_bytes,
                               void *stream) {
  return ctc_amd_windowed_best_path(kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride, label_length,
                                    logit_length, blank_index, nullptr, 0, B, T, V, U, score, tokens, label_index, first_frame, last_frame,
                                    label_score, workspace, workspace_bytes, stream);
}

static_assert(ctc::LONG_MAX_U == CTC_AMD_LONG_MAX_U && ctc::LONG_RING_FRAMES == CTC_AMD_LONG_FRAMES_MULTIPLE &&
              ctc::LONG_TF_DEFAULT == CTC_AMD_LONG_FRAMES_DEFAULT, "the tiled alignment's limits are the ABI's");

int ctc_amd_long_best_path_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, size_t *out_bytes) {
  return long_query<ctc::LongPlan>(kind, B, T, V, U, frames_per_tile, out_bytes,
                                   [=](ctc::LongPlan *plan) { return ctc::long_plan(B, T, U, frames_per_tile, plan); });
}

// The long-form entry points take CTC_AMD_LONG_MAX_U label positions: the label axis spans workgroups.
int ctc_amd_long_best_path(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                           const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                           int blank_index, int B, int T, int V, int U, int frames_per_tile, float *score, int32_t *tokens,
                           int32_t *label_index, int32_t *first_frame, int32_t *last_frame, void *workspace, size_t workspace_bytes,
                           void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false, CTC_AMD_LONG_MAX_U);
  if (!pre.go) return pre.rc;
  if (int rc = check_alignment(score, tokens, T, V)) return rc;
  ctc::LongPlan plan;
  if (!ctc::long_plan(B, T, U, frames_per_tile, &plan)) return bad_tiling(frames_per_tile, B, T, U);
  if (int rc = check_workspace(workspace, workspace_bytes, plan.total, NullWs::Refused)) return rc;
  CTC_TRY(ctc::run_align_long(pre.p, plan, static_cast<char *>(workspace), score, tokens, label_index, first_frame, last_frame,
                              static_cast<hipStream_t>(stream)), "long alignment launch");
  return CTC_AMD_OK;
}

int ctc_amd_long_wildcard_best_path_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, size_t *out_bytes) {
  return long_query<ctc::LongWildPlan>(kind, B, T, V, U, frames_per_tile, out_bytes,
                                       [=](ctc::LongWildPlan *plan) { return ctc::long_wild_plan(B, T, U, frames_per_tile, plan); });
}

// label_score, like the other per-label outputs, may be null.
int ctc_amd_long_windowed_best_path(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                    int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                    const int32_t *logit_length, int blank_index, const int32_t *frame_window, int window_stride, int B,
                                    int T, int V, int U, int frames_per_tile, float *score, int32_t *tokens, int32_t *label_index,
                                    int32_t *first_frame, int32_t *last_frame, float *label_score, void *workspace,
                                    size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false, CTC_AMD_LONG_MAX_U);
  if (!pre.go) return pre.rc;
  if (int rc = check_alignment(score, tokens, T, V)) return rc;
  if (int rc = check_window(frame_window, window_stride, U)) return rc;
  ctc::LongWildPlan plan;
  if (!ctc::long_wild_plan(B, T, U, frames_per_tile, &plan)) return bad_tiling(frames_per_tile, B, T, U);
  if (int rc = check_workspace(workspace, workspace_bytes, plan.total, NullWs::Refused)) return rc;
  CTC_TRY(ctc::run_align_long_wild(pre.p, plan, static_cast<char *>(workspace), score, tokens, label_index, first_frame, last_frame,
                                   label_score, static_cast<hipStream_t>(stream), frame_window, window_stride),
          "long wildcard alignment launch");
  return CTC_AMD_OK;
}

int ctc_amd_long_wildcard_best_path(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                    int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                    const int32_t *logit_length, int blank_index, int B, int T, int V, int U, int frames_per_tile,
                                    float *score, int32_t *tokens, int32_t *label_index, int32_t *first_frame, int32_t *last_frame,
                                    float *label_score, void *workspace, size_t workspace_bytes, void *stream) {
  return ctc_amd_long_windowed_best_path(kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride,
                                         label_length, logit_length, blank_index, nullptr, 0, B, T, V, U, frames_per_tile, score, tokens,
                                         label_index, first_frame, last_frame, label_score, workspace, workspace_bytes, stream);
}

static_assert(ctc::WILD_LOSS_WILDCARD == CTC_AMD_WILDCARD, "the loss kernel's wildcard label is the ABI's");
static_assert(ctc::WILD_LOSS_OPTIONAL == CTC_AMD_OPTIONAL_WILDCARD, "the loss kernel's optional wildcard label is the ABI's");

int ctc_amd_wildcard_loss_workspace_bytes(int kind, int B, int T, int V, int U, int want_grad, size_t *out_bytes) {
  if (int rc = check_query(kind, B, T, V, U, out_bytes)) return rc;
  *out_bytes = ctc::wild_loss_workspace_bytes(kind, B, T, U, want_grad != 0);
  return CTC_AMD_OK;
}

// The gradient's strides are looked at only when there is one; without one it needs no workspace today, so a null one passes.
// One body for ctc_amd_windowed_loss_grad and ctc_amd_optional_wildcard_loss_grad (which has no window).
static int wildcard_loss_grad_call(bool optional_wildcards, int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                   int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                   const int32_t *logit_length, int blank_index, const int32_t *frame_window, int window_stride,
                                   float wildcard_log_weight, int B, int T, int V, int U, const float *d_loss, float *loss, void *grad,
                                   int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t, void *workspace, size_t workspace_bytes,
                                   void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, logits_stride_b, logits_stride_t, grad_dtype, grad_stride_b, grad_stride_t};
  const Prelude pre = prelude(c, f, grad != nullptr);
  if (!pre.go) return pre.rc;
  if (int rc = check_wildcard_loss(wildcard_log_weight, loss, B, T, V, grad != nullptr)) return rc;
  if (int rc = check_window(frame_window, window_stride, U)) return rc;
  const size_t need = ctc::wild_loss_workspace_bytes(kind, B, T, U, grad != nullptr);
  if (int rc = check_workspace(workspace, workspace_bytes, need, NullWs::TakenIfUnneeded)) return rc;
  CTC_TRY(ctc::run_wild_loss(pre.p, wildcard_log_weight, d_loss, loss, grad, static_cast<char *>(workspace), static_cast<hipStream_t>(stream),
                             frame_window, window_stride, optional_wildcards), "wildcard loss launch");
  return CTC_AMD_OK;
}

int ctc_amd_windowed_loss_grad(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                               const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                               int blank_index, const int32_t *frame_window, int window_stride, float wildcard_log_weight, int B, int T,
                               int V, int U, const float *d_loss, float *loss, void *grad, int grad_dtype, int64_t grad_stride_b,
                               int64_t grad_stride_t, void *workspace, size_t workspace_bytes, void *stream) {
  return wildcard_loss_grad_call(false, kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride,
                                 label_length, logit_length, blank_index, frame_window, window_stride, wildcard_log_weight, B, T, V, U,
                                 d_loss, loss, grad, grad_dtype, grad_stride_b, grad_stride_t, workspace, workspace_bytes, stream);
}

// Optional wildcards: the counterpart's arguments, checks and workspace; CTC_AMD_OPTIONAL_WILDCARD is accepted in the labels.
int ctc_amd_optional_wildcard_loss_workspace_bytes(int kind, int B, int T, int V, int U, int want_grad, size_t *out_bytes) {
  return ctc_amd_wildcard_loss_workspace_bytes(kind, B, T, V, U, want_grad, out_bytes);
}

int ctc_amd_optional_wildcard_loss_grad(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                        int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                        const int32_t *logit_length, int blank_index, float wildcard_log_weight, int B, int T, int V, int U,
                                        const float *d_loss, float *loss, void *grad, int grad_dtype, int64_t grad_stride_b,
                                        int64_t grad_stride_t, void *workspace, size_t workspace_bytes, void *stream) {
  return wildcard_loss_grad_call(true, kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride,
                                 label_length, logit_length, blank_index, nullptr, 0, wildcard_log_weight, B, T, V, U, d_loss, loss, grad,
                                 grad_dtype, grad_stride_b, grad_stride_t, workspace, workspace_bytes, stream);
}

int ctc_amd_wildcard_loss_grad(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                               const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                               int blank_index, float wildcard_log_weight, int B, int T, int V, int U, const float *d_loss, float *loss,
                               void *grad, int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t, void *workspace,
                               size_t workspace_bytes, void *stream) {
  return ctc_amd_windowed_loss_grad(kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride, label_length,
                                    logit_length, blank_index, nullptr, 0, wildcard_log_weight, B, T, V, U, d_loss, loss, grad, grad_dtype,
                                    grad_stride_b, grad_stride_t, workspace, workspace_bytes, stream);
}

int ctc_amd_long_wildcard_loss_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, int want_grad, size_t *out_bytes) {
  return long_query<ctc::LongLossPlan>(kind, B, T, V, U, frames_per_tile, out_bytes, [=](ctc::LongLossPlan *plan) {
    return ctc::long_loss_plan(kind, B, T, U, frames_per_tile, want_grad != 0, plan);
  });
}

// The three long-form entry points with optional wildcards are their counterparts' bodies with the flag set:
// the same checks in the same order with the same words, and a plan that holds two more column buffers.
int ctc_amd_long_optional_wildcard_loss_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, int want_grad,
                                                        size_t *out_bytes) {
  return long_query<ctc::LongLossPlan>(kind, B, T, V, U, frames_per_tile, out_bytes, [=](ctc::LongLossPlan *plan) {
    return ctc::long_loss_plan(kind, B, T, U, frames_per_tile, want_grad != 0, plan, 1);
  });
}

int ctc_amd_long_optional_wildcard_loss_grad(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                             int64_t logits_stride_t, const int32_t *labels, int label_stride,
                                             const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                             float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                             const float *d_loss, float *loss, void *grad, int grad_dtype, int64_t grad_stride_b,
                                             int64_t grad_stride_t, void *workspace, size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, logits_stride_b, logits_stride_t, grad_dtype, grad_stride_b, grad_stride_t};
  return long_wildcard_loss_grad_impl(ctc::long_loss_plan, true, c, f, nullptr, 0, wildcard_log_weight, frames_per_tile, d_loss, loss, grad,
                                      workspace, workspace_bytes, stream);
}

int ctc_amd_long_optional_wildcard_loss_ckpt_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, int want_grad,
                                                             size_t *out_bytes) {
  return long_query<ctc::LongLossPlan>(kind, B, T, V, U, frames_per_tile, out_bytes, [=](ctc::LongLossPlan *plan) {
    return ctc::long_loss_ckpt_plan(kind, B, T, U, frames_per_tile, want_grad != 0, plan, 1);
  });
}

int ctc_amd_long_optional_wildcard_loss_grad_ckpt(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                                  int64_t logits_stride_t, const int32_t *labels, int label_stride,
                                                  const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                                  float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                                  const float *d_loss, float *loss, void *grad, int grad_dtype, int64_t grad_stride_b,
                                                  int64_t grad_stride_t, void *workspace, size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, logits_stride_b, logits_stride_t, grad_dtype, grad_stride_b, grad_stride_t};
  return long_wildcard_loss_grad_impl(ctc::long_loss_ckpt_plan, true, c, f, nullptr, 0, wildcard_log_weight, frames_per_tile, d_loss, loss,
                                      grad, workspace, workspace_bytes, stream);
}

// The three long-form windowed entry points are their counterparts with a frame window; the counterparts are they with none.
int ctc_amd_long_windowed_loss_grad(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                    int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                    const int32_t *logit_length, int blank_index, const int32_t *frame_window, int window_stride,
                                    float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile, const float *d_loss,
                                    float *loss, void *grad, int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t,
                                    void *workspace, size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, logits_stride_b, logits_stride_t, grad_dtype, grad_stride_b, grad_stride_t};
  return long_wildcard_loss_grad_impl(ctc::long_loss_plan, false, c, f, frame_window, window_stride, wildcard_log_weight, frames_per_tile, d_loss,
                                      loss, grad, workspace, workspace_bytes, stream);
}

int ctc_amd_long_wildcard_loss_grad(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                    int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                    const int32_t *logit_length, int blank_index, float wildcard_log_weight, int B, int T, int V, int U,
                                    int frames_per_tile, const float *d_loss, float *loss, void *grad, int grad_dtype,
                                    int64_t grad_stride_b, int64_t grad_stride_t, void *workspace, size_t workspace_bytes, void *stream) {
  return ctc_amd_long_windowed_loss_grad(kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride,
                                         label_length, logit_length, blank_index, nullptr, 0, wildcard_log_weight, B, T, V, U,
                                         frames_per_tile, d_loss, loss, grad, grad_dtype, grad_stride_b, grad_stride_t, workspace,
                                         workspace_bytes, stream);
}

int ctc_amd_long_wildcard_loss_ckpt_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, int want_grad,
                                                    size_t *out_bytes) {
  return long_query<ctc::LongLossPlan>(kind, B, T, V, U, frames_per_tile, out_bytes, [=](ctc::LongLossPlan *plan) {
    return ctc::long_loss_ckpt_plan(kind, B, T, U, frames_per_tile, want_grad != 0, plan);
  });
}

int ctc_amd_long_windowed_loss_grad_ckpt(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                         int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                         const int32_t *logit_length, int blank_index, const int32_t *frame_window, int window_stride,
                                         float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile, const float *d_loss,
                                         float *loss, void *grad, int grad_dtype, int64_t grad_stride_b, int64_t grad_stride_t,
                                         void *workspace, size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, logits_stride_b, logits_stride_t, grad_dtype, grad_stride_b, grad_stride_t};
  return long_wildcard_loss_grad_impl(ctc::long_loss_ckpt_plan, false, c, f, frame_window, window_stride, wildcard_log_weight, frames_per_tile,
                                      d_loss, loss, grad, workspace, workspace_bytes, stream);
}

int ctc_amd_long_wildcard_loss_grad_ckpt(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                         int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                         const int32_t *logit_length, int blank_index, float wildcard_log_weight, int B, int T, int V,
                                         int U, int frames_per_tile, const float *d_loss, float *loss, void *grad, int grad_dtype,
                                         int64_t grad_stride_b, int64_t grad_stride_t, void *workspace, size_t workspace_bytes,
                                         void *stream) {
  return ctc_amd_long_windowed_loss_grad_ckpt(kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride,
                                              label_length, logit_length, blank_index, nullptr, 0, wildcard_log_weight, B, T, V, U,
                                              frames_per_tile, d_loss, loss, grad, grad_dtype, grad_stride_b, grad_stride_t, workspace,
                                              workspace_bytes, stream);
}

int ctc_amd_label_posterior_workspace_bytes(int kind, int B, int T, int V, int U, size_t *out_bytes) {
  return ctc_amd_wildcard_loss_workspace_bytes(kind, B, T, V, U, 1, out_bytes);
}

// One body for ctc_amd_windowed_label_posterior and ctc_amd_optional_wildcard_label_posterior (which has no window).
static int label_posterior_call(bool optional_wildcards, int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                const int32_t *logit_length, int blank_index, const int32_t *frame_window, int window_stride,
                                float wildcard_log_weight, int B, int T, int V, int U, float *loss, float *label_posterior,
                                float *blank_posterior, float *duration, float *expected_frame, void *workspace, size_t workspace_bytes,
                                void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, logits_stride_b, logits_stride_t, CTC_AMD_F32, logits_stride_b, logits_stride_t};  // (no gradient: nothing reads the second half)
  const Prelude pre = prelude(c, f, false);
  if (!pre.go) return pre.rc;
  if (int rc = check_wildcard_weight(wildcard_log_weight)) return rc;
  if (!loss || (T > 0 && U > 0 && !label_posterior) || (T > 0 && !blank_posterior))
    return fail(CTC_AMD_EINVAL, "null loss / label_posterior / blank_posterior pointer");
  if (!duration != !expected_frame) return fail(CTC_AMD_EINVAL, "duration and expected_frame must both be given or both be NULL");
  if (int rc = check_vocab(V, " of the label posteriors")) return rc;
  if (int rc = check_window(frame_window, window_stride, U)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, ctc::wild_loss_workspace_bytes(kind, B, T, U, true), NullWs::Refused)) return rc;
  CTC_TRY(ctc::run_label_posterior(pre.p, wildcard_log_weight, loss, label_posterior, blank_posterior, duration, expected_frame,
                                   static_cast<char *>(workspace), static_cast<hipStream_t>(stream), frame_window, window_stride,
                                   optional_wildcards),
          "label posterior launch");
  return CTC_AMD_OK;
}

int ctc_amd_windowed_label_posterior(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                     int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                     const int32_t *logit_length, int blank_index, const int32_t *frame_window, int window_stride,
                                     float wildcard_log_weight, int B, int T, int V, int U, float *loss, float *label_posterior,
                                     float *blank_posterior, float *duration, float *expected_frame, void *workspace,
                                     size_t workspace_bytes, void *stream) {
  return label_posterior_call(false, kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride, label_length,
                              logit_length, blank_index, frame_window, window_stride, wildcard_log_weight, B, T, V, U, loss,
                              label_posterior, blank_posterior, duration, expected_frame, workspace, workspace_bytes, stream);
}

int ctc_amd_optional_wildcard_label_posterior_workspace_bytes(int kind, int B, int T, int V, int U, size_t *out_bytes) {
  return ctc_amd_label_posterior_workspace_bytes(kind, B, T, V, U, out_bytes);
}

int ctc_amd_optional_wildcard_label_posterior(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                              int64_t logits_stride_t, const int32_t *labels, int label_stride,
                                              const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                              float wildcard_log_weight, int B, int T, int V, int U, float *loss, float *label_posterior,
                                              float *blank_posterior, float *duration, float *expected_frame, void *workspace,
                                              size_t workspace_bytes, void *stream) {
  return label_posterior_call(true, kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride, label_length,
                              logit_length, blank_index, nullptr, 0, wildcard_log_weight, B, T, V, U, loss, label_posterior,
                              blank_posterior, duration, expected_frame, workspace, workspace_bytes, stream);
}

int ctc_amd_label_posterior(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                            const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                            int blank_index, float wildcard_log_weight, int B, int T, int V, int U, float *loss, float *label_posterior,
                            float *blank_posterior, float *duration, float *expected_frame, void *workspace, size_t workspace_bytes,
                            void *stream) {
  return ctc_amd_windowed_label_posterior(kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride,
                                          label_length, logit_length, blank_index, nullptr, 0, wildcard_log_weight, B, T, V, U, loss,
                                          label_posterior, blank_posterior, duration, expected_frame, workspace, workspace_bytes, stream);
}

int ctc_amd_long_label_posterior_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile, size_t *out_bytes) {
  return long_query<ctc::LongPostPlan>(kind, B, T, V, U, frames_per_tile, out_bytes,
                                       [=](ctc::LongPostPlan *plan) { return ctc::long_post_plan(kind, B, T, U, frames_per_tile, plan); });
}

// It begins like ctc_amd_long_wildcard_loss_grad with a gradient, whose messages it gives (the row stage always runs); its own
// outputs come behind that.
// One body for ctc_amd_long_windowed_label_posterior and ctc_amd_long_optional_wildcard_label_posterior (which has no window).
static int long_label_posterior_call(bool optional_wildcards, int kind, int wrt, const void *logits, int logits_dtype,
                                     int64_t logits_stride_b, int64_t logits_stride_t, const int32_t *labels, int label_stride,
                                     const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                     const int32_t *frame_window, int window_stride, float wildcard_log_weight, int B, int T, int V, int U,
                                     int frames_per_tile, float *loss, float *label_posterior, float *blank_posterior, float *duration,
                                     float *expected_frame, float *peak_posterior, int32_t *peak_frame, void *workspace,
                                     size_t workspace_bytes, void *stream) {
  const Common c{kind, wrt, logits, labels, label_stride, label_length, logit_length, blank_index, B, T, V, U};
  const Format f{logits_dtype, logits_stride_b, logits_stride_t, CTC_AMD_F32, logits_stride_b, logits_stride_t};  // (no gradient: nothing reads the second half)
  const Prelude pre = prelude(c, f, false, CTC_AMD_LONG_MAX_U);
  if (!pre.go) return pre.rc;
  if (int rc = check_wildcard_loss(wildcard_log_weight, loss, B, T, V, true)) return rc;
  if (T > 0 && !blank_posterior) return fail(CTC_AMD_EINVAL, "null blank_posterior pointer");
  if (!duration != !expected_frame) return fail(CTC_AMD_EINVAL, "duration and expected_frame must both be given or both be NULL");
  if (!peak_posterior != !peak_frame) return fail(CTC_AMD_EINVAL, "peak_posterior and peak_frame must both be given or both be NULL");
  ctc::LongPostPlan plan;
  if (!ctc::long_post_plan(kind, B, T, U, frames_per_tile, &plan, optional_wildcards ? 1 : 0)) return bad_tiling(frames_per_tile, B, T, U);
  if (int rc = check_window(frame_window, window_stride, U)) return rc;
  if (int rc = check_workspace(workspace, workspace_bytes, plan.total, NullWs::Refused)) return rc;
  CTC_TRY(ctc::run_long_label_posterior(pre.p, plan, wildcard_log_weight, loss, label_posterior, blank_posterior, duration, expected_frame,
                                        peak_posterior, peak_frame, static_cast<char *>(workspace), static_cast<hipStream_t>(stream),
                                        frame_window, window_stride, optional_wildcards),
          "long label posterior launch");
  return CTC_AMD_OK;
}

int ctc_amd_long_windowed_label_posterior(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                          int64_t logits_stride_t, const int32_t *labels, int label_stride, const int32_t *label_length,
                                          const int32_t *logit_length, int blank_index, const int32_t *frame_window, int window_stride,
                                          float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile, float *loss,
                                          float *label_posterior, float *blank_posterior, float *duration, float *expected_frame,
                                          float *peak_posterior, int32_t *peak_frame, void *workspace, size_t workspace_bytes,
                                          void *stream) {
  return long_label_posterior_call(false, kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride,
                                   label_length, logit_length, blank_index, frame_window, window_stride, wildcard_log_weight, B, T, V, U,
                                   frames_per_tile, loss, label_posterior, blank_posterior, duration, expected_frame, peak_posterior,
                                   peak_frame, workspace, workspace_bytes, stream);
}

int ctc_amd_long_optional_wildcard_label_posterior_workspace_bytes(int kind, int B, int T, int V, int U, int frames_per_tile,
                                                                   size_t *out_bytes) {
  return long_query<ctc::LongPostPlan>(kind, B, T, V, U, frames_per_tile, out_bytes,
                                       [=](ctc::LongPostPlan *plan) { return ctc::long_post_plan(kind, B, T, U, frames_per_tile, plan, 1); });
}

int ctc_amd_long_optional_wildcard_label_posterior(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b,
                                                   int64_t logits_stride_t, const int32_t *labels, int label_stride,
                                                   const int32_t *label_length, const int32_t *logit_length, int blank_index,
                                                   float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile,
                                                   float *loss, float *label_posterior, float *blank_posterior, float *duration,
                                                   float *expected_frame, float *peak_posterior, int32_t *peak_frame, void *workspace,
                                                   size_t workspace_bytes, void *stream) {
  return long_label_posterior_call(true, kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride,
                                   label_length, logit_length, blank_index, nullptr, 0, wildcard_log_weight, B, T, V, U, frames_per_tile,
                                   loss, label_posterior, blank_posterior, duration, expected_frame, peak_posterior, peak_frame,
                                   workspace, workspace_bytes, stream);
}

int ctc_amd_long_label_posterior(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                                 const int32_t *labels, int label_stride, const int32_t *label_length, const int32_t *logit_length,
                                 int blank_index, float wildcard_log_weight, int B, int T, int V, int U, int frames_per_tile, float *loss,
                                 float *label_posterior, float *blank_posterior, float *duration, float *expected_frame,
                                 float *peak_posterior, int32_t *peak_frame, void *workspace, size_t workspace_bytes, void *stream) {
  return ctc_amd_long_windowed_label_posterior(kind, wrt, logits, logits_dtype, logits_stride_b, logits_stride_t, labels, label_stride,
                                               label_length, logit_length, blank_index, nullptr, 0, wildcard_log_weight, B, T, V, U,
                                               frames_per_tile, loss, label_posterior, blank_posterior, duration, expected_frame,
                                               peak_posterior, peak_frame, workspace, workspace_bytes, stream);
}

int ctc_amd_edit_distance_workspace_bytes(int B, int N, int R, size_t *out_bytes) {
  if (int rc = check_out_bytes(out_bytes)) return rc;
  if (int rc = check_edit_sizes(B, R, MAX_U)) return rc;
  if (int rc = check_edit_pairs(B, N)) return rc;
  *out_bytes = 0;
  return CTC_AMD_OK;
}

// No logits, so no prelude: the sizes, B == 0, then N and the number of pairs, the strides, the pointers.  No workspace: the
// pointer may be null.
int ctc_amd_edit_distance(const int32_t *hyp, int hyp_stride, const int32_t *hyp_length, const int32_t *ref, int ref_stride,
                          const int32_t *ref_length, int B, int N, int R, int32_t *distance, void *workspace, size_t workspace_bytes,
                          void *stream) {
  (void)workspace;
  (void)workspace_bytes;
  if (int rc = check_edit_sizes(B, R, MAX_U)) return rc;
  if (B == 0) return CTC_AMD_OK;
  if (int rc = check_edit_pairs(B, N)) return rc;
  if (int rc = check_edit_strides(hyp_stride, ref_stride)) return rc;
  if (hyp_stride > CTC_AMD_EDIT_MAX_STRIDE) return fail(CTC_AMD_EINVAL, "hyp_stride=%d exceeds the supported maximum %d", hyp_stride, CTC_AMD_EDIT_MAX_STRIDE);
  if (!hyp_length || !ref_length) return fail(CTC_AMD_EINVAL, "null length pointer");
  if (hyp_stride > 0 && !hyp) return fail(CTC_AMD_EINVAL, "null hyp pointer");
  if (ref_stride > 0 && !ref) return fail(CTC_AMD_EINVAL, "null ref pointer");
  if (!distance) return fail(CTC_AMD_EINVAL, "null distance pointer");
  CTC_TRY(ctc::run_edit_distance(hyp, hyp_stride, hyp_length, ref, ref_stride, ref_length, B, N, R, distance,
                                 static_cast<hipStream_t>(stream)), "edit distance launch");
  return CTC_AMD_OK;
}

int ctc_amd_edit_counts_workspace_bytes(int B, int N, int R, int hyp_stride, int rows_per_tile, size_t *out_bytes) {
  if (int rc = check_out_bytes(out_bytes)) return rc;
  if (int rc = check_edit_sizes(B, R, CTC_AMD_LONG_MAX_U)) return rc;
  if (int rc = check_edit_pairs(B, N)) return rc;
  ctc::EditCountsPlan plan;
  if (int rc = check_edit_counts_tiling(B, N, R, hyp_stride, rows_per_tile, &plan)) return rc;
  *out_bytes = plan.total;
  return CTC_AMD_OK;
}

// As ctc_amd_edit_distance, with rows_per_tile and the launch grid behind the strides, and a workspace.
int ctc_amd_edit_counts(const int32_t *hyp, int hyp_stride, const int32_t *hyp_length, const int32_t *ref, int ref_stride,
                        const int32_t *ref_length, int B, int N, int R, int rows_per_tile, int32_t *counts, void *workspace,
                        size_t workspace_bytes, void *stream) {
  if (int rc = check_edit_sizes(B, R, CTC_AMD_LONG_MAX_U)) return rc;
  if (B == 0) return CTC_AMD_OK;
  if (int rc = check_edit_pairs(B, N)) return rc;
  if (int rc = check_edit_strides(hyp_stride, ref_stride)) return rc;
  ctc::EditCountsPlan plan;
  if (int rc = check_edit_counts_tiling(B, N, R, hyp_stride, rows_per_tile, &plan)) return rc;
  if (!hyp_length || !ref_length) return fail(CTC_AMD_EINVAL, "null length pointer");
  if (hyp_stride > 0 && !hyp) return fail(CTC_AMD_EINVAL, "null hyp pointer");
  if (ref_stride > 0 && !ref) return fail(CTC_AMD_EINVAL, "null ref pointer");
  if (!counts) return fail(CTC_AMD_EINVAL, "null counts pointer");
  if (int rc = check_workspace(workspace, workspace_bytes, plan.total, NullWs::Refused)) return rc;
  CTC_TRY(ctc::run_edit_counts(hyp, hyp_stride, hyp_length, ref, ref_stride, ref_length, N, plan, counts, static_cast<char *>(workspace),
                               static_cast<hipStream_t>(stream)), "edit counts launch");
  return CTC_AMD_OK;
}

int ctc_amd_prefix_workspace_bytes(int B, int T, int V, int N, size_t *rows_bytes, size_t *state_bytes) {
  if (!rows_bytes || !state_bytes) return fail(CTC_AMD_EINVAL, "rows_bytes or state_bytes is null");
  if (B < 0 || T < 0 || V <= 0) return fail(CTC_AMD_EINVAL, "negative size: B=%d T=%d V=%d", B, T, V);
  if (int rc = check_prefix(B, V, N)) return rc;
  *rows_bytes = ctc::prefix_rows_bytes(B, T);
  *state_bytes = ctc::prefix_state_bytes(B, T, N);
  return CTC_AMD_OK;
}

// No labels, as in ctc_amd_greedy_decode, and no blank: column 0 stands in.  Its buffer has a message of its own.
int ctc_amd_prefix_rows(const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                        const int32_t *logit_length, int B, int T, int V, void *rows, size_t rows_bytes, void *stream) {
  const Common c{CTC_AMD_CLASSIC, CTC_AMD_WRT_LOGITS, logits, nullptr, 0, logit_length, logit_length, 0, B, T, V, 0};
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false);
  if (!pre.go) return pre.rc;
  if (int rc = check_prefix(B, V, 1)) return rc;
  if (int rc = check_row_grid(B, T, 4)) return rc;
  const size_t need = ctc::prefix_rows_bytes(B, T);
  if (rows_bytes < need || (need > 0 && !rows)) return fail(CTC_AMD_EWORKSPACE, "rows buffer too small: %zu < %zu", rows_bytes, need);
  CTC_TRY(ctc::run_prefix_rows(pre.p, rows, static_cast<hipStream_t>(stream)), "prefix rows launch");
  return CTC_AMD_OK;
}

int ctc_amd_prefix_extend(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                          const int32_t *logit_length, int blank_index, int B, int T, int V, int N, const void *rows, size_t rows_bytes,
                          const void *state_in, const int32_t *last_token_in, const int32_t *length_in, const int32_t *parent,
                          const int32_t *token, void *state_out, size_t state_bytes, int32_t *last_token_out, int32_t *length_out,
                          float *full_score, void *stream) {
  const Common c{kind, wrt, logits, nullptr, 0, logit_length, logit_length, blank_index, B, T, V, 0};
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false);
  if (!pre.go) return pre.rc;
  if (int rc = check_prefix_step(pre.p, N, rows, rows_bytes)) return rc;
  if (!parent || !token || !state_out || !last_token_out || !length_out || !full_score)
    return fail(CTC_AMD_EINVAL, "null parent / token / state_out / last_token_out / length_out / full_score pointer");
  if (state_in && (!last_token_in || !length_in)) return fail(CTC_AMD_EINVAL, "state_in without last_token_in / length_in");
  if (state_in == state_out) return fail(CTC_AMD_EINVAL, "state_out must not be state_in");
  const size_t need = ctc::prefix_state_bytes(B, T, N);
  if (state_bytes < need) return fail(CTC_AMD_EWORKSPACE, "state buffer too small: %zu < %zu", state_bytes, need);
  CTC_TRY(ctc::run_prefix_extend(pre.p, N, rows, static_cast<const double *>(state_in), last_token_in, length_in, parent, token,
                                 static_cast<double *>(state_out), last_token_out, length_out, full_score,
                                 static_cast<hipStream_t>(stream)), "prefix extend launch");
  return CTC_AMD_OK;
}

int ctc_amd_prefix_score(int kind, int wrt, const void *logits, int logits_dtype, int64_t logits_stride_b, int64_t logits_stride_t,
                         const int32_t *logit_length, int blank_index, int B, int T, int V, int N, const void *rows, size_t rows_bytes,
                         const void *state, size_t state_bytes, const int32_t *last_token, const int32_t *length, float *score,
                         void *stream) {
  const Common c{kind, wrt, logits, nullptr, 0, logit_length, logit_length, blank_index, B, T, V, 0};
  const Prelude pre = prelude(c, Format::of_logits(logits_dtype, logits_stride_b, logits_stride_t), false);
  if (!pre.go) return pre.rc;
  if (int rc = check_prefix_step(pre.p, N, rows, rows_bytes)) return rc;
  if (!state || !last_token || !length || !score) return fail(CTC_AMD_EINVAL, "null state / last_token / length / score pointer");
  const size_t need = ctc::prefix_state_bytes(B, T, N);
  if (state_bytes < need) return fail(CTC_AMD_EWORKSPACE, "state buffer too small: %zu < %zu", state_bytes, need);
  CTC_TRY(ctc::run_prefix_score(pre.p, N, rows, static_cast<const double *>(state), last_token, length, score,
                                static_cast<hipStream_t>(stream)), "prefix score launch");
  return CTC_AMD_OK;
}

}  // extern "C"
