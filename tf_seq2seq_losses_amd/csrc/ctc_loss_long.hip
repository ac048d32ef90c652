// Long-form CTC loss and gradient with wildcard labels on both lattices: ctc_amd_long_wildcard_loss_grad (include/ctc_amd.h),
// DESIGN.md section 5.20.  The contract of ctc_amd_wildcard_loss_grad for U <= CTC_AMD_LONG_MAX_U label positions.
//
// The sum-product lattice of ctc_wild_loss.hip (float64 base-2 log state with a true -inf, the same chain step, posteriors and row
// stage) on the tiles of ctc_align_long_wild.hip (label blocks of UB = 1024 positions x time blocks of TF frames, one launch per
// anti-diagonal of tiles, the order of the launches on the stream the only dependency).  Both units stay as they are: what is
// file-local there is repeated here.
//   alpha tile   <KIND, MODE>; wave 0 the chain at NL = 16, waves 1..4 the producers, one frame each through a ring of 4 frames.
//                Row in / row out per (utterance, label block); column in / column out the pair (O, C) (simplified: S) of position
//                k * UB - 1 BEFORE every frame, stored per frame by the left neighbour.  The `allow` bit of position k * UB sees
//                label[k * UB - 1].  Label block 0 takes the row statistics (x[blank], max, log2 sum exp) once per frame and keeps
//                them per frame for the blocks to its right, which run on later launches.  MODE 1 also stores the chain's state of
//                every frame per (b, k, t): the saved row of ctc_wild_loss.hip, one per label block (classic AFTER the frame,
//                simplified BEFORE it, the start state in block 0).
//   finish       log2 Z from the row buffer of block (L - 1) / UB (L = 0: the start state): loss[b], log2 Z, a feasibility word.
//   beta tile    the reverse anti-diagonals: tile (k, j) after (k + 1, j) and (k, j + 1).  What MODE 2 of wild_loss_kernel gets
//                from the next lane comes across the block boundary per frame through a column: the worth of entering position
//                (k + 1) * UB with that frame (beta plus the emission), stored by lane 0 of the right neighbour and staged through
//                LDS by the producers; the `allow` bit of the skip into it is read off the labels.  Beta rows go back in time
//                through a row buffer.  Per frame the chain reads the saved alpha row, forms 2^(alpha + beta - log2 Z) and writes
//                the posteriors as float32 pairs over the slots it has read (MODE 2's slot convention).  Simplified: alpha of
//                position k * UB - 1 before the frame is the alpha column of the forward sweep.
//   row stage    one wavefront per (b, t) looping over the label blocks of that frame: wild_grad_row_kernel.
// ctc_amd_long_wildcard_loss_grad_ckpt is the same kernels on another workspace: alpha MODE 2 is MODE 0 with
// a row buffer per tile (the checkpoints), MODE 3 runs a tile again from its checkpoint on the backward sweep and saves its rows into
// a ring of min(K, J) time blocks, the beta tile and the row stage read the ring, and the row stage runs per time block.  Where a
// checkpoint and a saved row live is long_loss_ckpt_index / long_loss_row_index (ctc_loss_long_plan.h) in both layouts.
// ctc_amd_long_label_posterior is that schedule with the posterior stage in the row stage's place: the ring
// rows of a time block become label_posterior / blank_posterior rows and, carried from block to block, the per-position sums and peaks.
// Frame windows (WIN; ctc_amd_long_windowed_loss_grad / _grad_ckpt / _label_posterior): every lane holds the
// (first, last) frames of its own NL positions, and the producers of both tiles store -inf for a position's slot at an absolute frame
// outside its pair -- in a wildcard's slot (which holds -inf otherwise and is never read) the gate 0 / -inf that the chain adds to the
// wave-uniform e_w.  MODE 3 carries the gate of the forward sweep, so its saved rows are that sweep's bits.  Nothing behind the ring
// knows of windows: the row statistics, columns, rows, checkpoints, the skip tests (a window only takes frames away), the finish
// kernels, the row stage and the posterior stage are those of the unwindowed call.
// Optional wildcards (OPT, never with WIN; ctc_amd_long_optional_wildcard_loss_grad / _grad_ckpt / _label_posterior, DESIGN.md section
// 5.27): the two-back step of ctc_wild_loss.hip at NL = 16 inside a tile; across a label block a second alpha column (position
// k * UB - 2 before every frame) and a second beta column (the worth of entering position (k + 1) * UB + 1 with the frame); the tile's
// labels reach from k * UB - 2 to k * UB + UB + 1, and whether a -3 is optional or half of a bad pair is read off the labels themselves;
// behind an optional last position the finish kernels and the first beta tiles take position L - 2 as an end state too; the tiles that
// run are long_loss_tile_active_opt's.  Where OPT is off, the source is the parent's expression for expression: the same device code.
// Which tiles run is long_loss_tile_active (ctc_loss_long_plan.h), asked by all of them; nothing unwritten is read.  No workgroup
// waits for another: no flags, no cooperative launch, no floating-point atomics, vector stores only, one writer per element.
#include "ctc_loss_long.h"

#include <type_traits>

namespace ctc {
namespace {

constexpr int NL = LONG_NL, UB = LONG_UB, RW = LONG_ROW_DOUBLES;
constexpr int LL_PW = 4;                      // producer wavefronts
constexpr int LL_THREADS = 64 * (1 + LL_PW);  // + the chain
constexpr int F = 4096 / UB;                  // frames per ring block
static_assert(F == LONG_RING_FRAMES && F == LL_PW, "one frame per producer wavefront and ring block");
constexpr int RS = UB + 4;  // ring row: UB label emissions, then x[blank], the row max, log2 sum exp(x - max)
constexpr double LOG2E_D = 1.44269504088896340736;

__device__ __forceinline__ float4 ll_row_load4(const char *row, int k, int dt) {
  if (dt == 0) return *reinterpret_cast<const float4 *>(row + (size_t)k * 4);
  const uint2 u = *reinterpret_cast<const uint2 *>(row + (size_t)k * 2);
  return make_float4(h16_to_f32((unsigned short)(u.x & 0xffffu), dt), h16_to_f32((unsigned short)(u.x >> 16), dt),
                     h16_to_f32((unsigned short)(u.y & 0xffffu), dt), h16_to_f32((unsigned short)(u.y >> 16), dt));
}
// the same four elements one by one (unaligned rows, V no multiple of 4): -inf past the row, which adds nothing to either statistic
__device__ __forceinline__ float4 ll_row_load4_elem(const char *row, int k, int V, int dt) {
  const float ninf = -__builtin_inff();
  return make_float4(row_load1(row, k, dt), k + 1 < V ? row_load1(row, k + 1, dt) : ninf, k + 2 < V ? row_load1(row, k + 2, dt) : ninf,
                     k + 3 < V ? row_load1(row, k + 3, dt) : ninf);
}
// running (max, sum of exp(x - max)) of one lane: four more elements (both access paths end here: identical bits)
__device__ __forceinline__ void ll_stat_add4(float &m, float &s, const float4 v) {
  const float mn = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
  s = s * fexp2((m - mn) * LOG2E) +
      ((fexp2((v.x - mn) * LOG2E) + fexp2((v.y - mn) * LOG2E)) + (fexp2((v.z - mn) * LOG2E) + fexp2((v.w - mn) * LOG2E)));
  m = mn;
}

// base-2 log(2^a + 2^b [+ 2^c]) of float64 operands that may be -inf (log 0): differences against the maximum, or against 0
// when every operand is -inf
__device__ __forceinline__ double ll_lse(double a, double b) {
  const double m = fmax(a, b);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2(fexp2((float)(a - mm)) + fexp2((float)(b - mm)));
}
__device__ __forceinline__ double ll_lse(double a, double b, double c) {
  const double m = fmax(fmax(a, b), c);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2((fexp2((float)(a - mm)) + fexp2((float)(b - mm))) + fexp2((float)(c - mm)));
}

// ... four and five operands (OPT): the further terms are added behind the first three, so operands of -inf there leave the bits
// of the three-operand result as they are
__device__ __forceinline__ double ll_lse(double a, double b, double c, double d) {
  const double m = fmax(fmax(a, b), fmax(c, d));
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2(((fexp2((float)(a - mm)) + fexp2((float)(b - mm))) + fexp2((float)(c - mm))) + fexp2((float)(d - mm)));
}
__device__ __forceinline__ double ll_lse(double a, double b, double c, double d, double e) {
  const double m = fmax(fmax(fmax(a, b), fmax(c, d)), e);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2((((fexp2((float)(a - mm)) + fexp2((float)(b - mm))) + fexp2((float)(c - mm))) + fexp2((float)(d - mm))) +
                            fexp2((float)(e - mm)));
}

struct LongLossWs {  // device pointers into the workspace (LongLossPlan offsets)
  double *col, *row;
  float *stat;
  double *logp;
  int *flag;
  double *colb, *rowb, *rows;
};
struct LongLossWsOpt : LongLossWs {  // what the OPT tiles take in its place
  double *col2, *colb2;  // the second columns (position k * UB - 2; entering position (k + 1) * UB + 1)
};
template <bool OPT> using LlWsArg = std::conditional_t<OPT, LongLossWsOpt, LongLossWs>;

// what a ring row says about its frame, in the lattice's units (base-2 logarithms of lp)
struct LlFrame {
  double Md, nl2s, eb, ew;
};
__device__ __forceinline__ LlFrame ll_frame_of(const float *r, bool lpin, double w2) {
  const float4 sv = *reinterpret_cast<const float4 *>(r + UB);
  LlFrame fr;
  // logits: lp = x - max - ln sum; log-probabilities: lp = x
  fr.Md = lpin ? 0.0 : (double)sv.y;
  fr.nl2s = lpin ? 0.0 : -(double)sv.z;
  fr.eb = fma((double)sv.x - fr.Md, LOG2E_D, fr.nl2s);
  // e_w = w + ln sum_k exp(lp[t, k]): w for logits, w + LSE_t for log-probabilities; a row of -inf emits nothing
  fr.ew = sv.z == __builtin_inff() ? -__builtin_inf() : lpin ? w2 + fma((double)sv.y, LOG2E_D, (double)sv.z) : w2;
  return fr;
}

// OPT: what position g of a transcript of L labels is when its label is LONG_LOSS_OPTIONAL: an optional wildcard, or, beside
// another one, a bad label (-1: no emission, no skip).  Asked of the labels themselves, so every tile, the finish kernels and the
// stages behind them reach the same verdict wherever a block boundary falls
__device__ __forceinline__ int ll_optional_class(const Problem &p, const int32_t *lr, int g, int L) {
  const bool pair = (g > 0 && label_at(p, lr, g - 1) == LONG_LOSS_OPTIONAL) || (g + 1 < L && label_at(p, lr, g + 1) == LONG_LOSS_OPTIONAL);
  return pair ? -1 : LONG_LOSS_OPTIONAL;
}
// OPT: the last position is an optional wildcard, so the states before it end the utterance too
__device__ __forceinline__ bool ll_last_optional(const Problem &p, int b, int L) {
  const int32_t *const lr = label_row(p, b);
  return L > 0 && label_at(p, lr, L - 1) == LONG_LOSS_OPTIONAL && ll_optional_class(p, lr, L - 1, L) == LONG_LOSS_OPTIONAL;
}

// the validated labels of positions k * UB - 1 .. k * UB + n - 2 into lab_s[0 .. n - 1] (-1: no emission)
__device__ __forceinline__ void ll_labels(const Problem &p, int b, int k, int L, int n, int *lab_s) {
  for (int i = threadIdx.x; i < n; i += LL_THREADS) {
    const int g = k * UB + i - 1;
    int tok = -1;
    if (g >= 0 && g < L) tok = label_at(p, label_row(p, b), g);
    lab_s[i] = tok == LONG_LOSS_WILDCARD ? LONG_LOSS_WILDCARD : emits(p, tok) ? tok : -1;
  }
}
// OPT: ... of positions k * UB - 2 .. k * UB + n - 3, an optional wildcard classed by ll_optional_class
__device__ __forceinline__ void ll_labels_opt(const Problem &p, int b, int k, int L, int n, int *lab_s) {
  for (int i = threadIdx.x; i < n; i += LL_THREADS) {
    const int g = k * UB + i - 2;
    int tok = -1;
    if (g >= 0 && g < L) tok = label_at(p, label_row(p, b), g);
    int cls = tok == LONG_LOSS_WILDCARD ? LONG_LOSS_WILDCARD : emits(p, tok) ? tok : -1;
    if (tok == LONG_LOSS_OPTIONAL) cls = ll_optional_class(p, label_row(p, b), g, L);
    lab_s[i] = cls;
  }
}
// which tiles run, OPT or not (ctc_loss_long_plan.h): the existing kernels call the existing predicates
template <bool OPT>
__device__ __forceinline__ bool ll_tile_active(int Tb, int L, int k, int j, int TF) {
  if constexpr (OPT) return long_loss_tile_active_opt(Tb, L, k, j, TF);
  else return long_loss_tile_active(Tb, L, k, j, TF);
}
// OPT: a wildcard of either kind
template <bool OPT>
__device__ __forceinline__ bool ll_is_wild(int tok) {
  return tok == LONG_LOSS_WILDCARD || (OPT && tok == LONG_LOSS_OPTIONAL);
}
// OPT: bit q of `skip` = the position before k * UB + i0 + q is an optional wildcard, so this one may also be entered from two
// positions back (position -1: the start state); bit q of `skipo` = (classic) ... from the open state there too.  lab_s holds the
// positions from k * UB - 2 on
template <int KIND, int NQ>
__device__ __forceinline__ void ll_skip_bits(const int *lab_s, int k, int i0, unsigned &skip, unsigned &skipo) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int i = i0 + q, g = k * UB + i;
    if (g >= 1 && lab_s[2 + i - 1] == LONG_LOSS_OPTIONAL) {
      skip |= 1u << q;
      const int a = lab_s[2 + i], c = lab_s[2 + i - 2];
      if (KIND == 0 && g >= 2 && (a != c || ll_is_wild<true>(a) || ll_is_wild<true>(c))) skipo |= 1u << q;
    }
  }
}

template <int KIND, int MODE, bool WIN, bool OPT>
__global__ __launch_bounds__(LL_THREADS) void loss_long_alpha_kernel(const Problem p, const double w2, const LlWsArg<OPT> w, int K, int TF,
                                                                     int d, int k_lo, int count, const int32_t *__restrict__ win,
                                                                     int wstride) {
  constexpr int NS = (KIND == 0 ? 2 : 1) * NL;  // doubles of a saved row per lane
  constexpr int SRD = long_loss_row_doubles(KIND);
  constexpr bool CKPT = MODE >= 2;               // row in / row out: the checkpoints of tiles (k, j - 1) / (k, j)
  constexpr bool SAVE = MODE == 1 || MODE == 3;  // the chain's state of every frame is stored
  constexpr bool REDO = MODE == 3;               // the forward sweep has run: nothing but the saved rows is written
  static_assert(!(WIN && OPT), "frame windows and optional wildcards are not combined");
  constexpr int LB = OPT ? 2 : 1;                // lab_s[LB + i]: position k * UB + i
  const double NINF = -__builtin_inf();
  __shared__ __attribute__((aligned(16))) float ring[2 * F * RS];
  __shared__ int lab_s[UB + LB];  // positions k * UB - LB .. k * UB + UB - 1
  __shared__ double col_s[2][F][2 * LB];  // (OPT: behind the pair of position k * UB - 1 that of k * UB - 2)

  const int b = blockIdx.x / count, k = k_lo + blockIdx.x % count, j = d - k;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = p.T, V = p.V, blank = p.blank, dt = p.xdtype;
  const bool lpin = p.wrt != 0;  // log-probability input
  const int Tb = frame_count(p, b);
  const int L = label_count(p, b);
  if (too_many_labels(p, L) || !ll_tile_active<OPT>(Tb, L, k, j, TF)) return;
  if (REDO && w.flag[b] == 0) return;  // (as the beta tile: an infeasible utterance has no posteriors, and nothing reads its rows)
  const int t_lo = j * TF;                           // (J * TF < T + TF: no overflow)
  const int t_hi = Tb - t_lo < TF ? Tb : t_lo + TF;  // one past the tile's last frame
  const bool fresh = OPT ? long_loss_alpha_fresh_opt(k, j, TF) : long_loss_alpha_fresh(k, j, TF);
  const bool has_right = long_loss_has_right(L, k);

  if constexpr (OPT) ll_labels_opt(p, b, k, L, UB + LB, lab_s);
  else ll_labels(p, b, k, L, UB + LB, lab_s);
  __syncthreads();

  int lab[NL];
  unsigned wild = 0;  // bit q = position k * UB + lane * NL + q is a wildcard (OPT: of either kind)
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    lab[q] = lab_s[LB + lane * NL + q];
    if constexpr (OPT) {
      if (ll_is_wild<true>(lab[q])) wild |= 1u << q;
    } else {
      if (lab[q] == LONG_LOSS_WILDCARD) wild |= 1u << q;
    }
  }
  [[maybe_unused]] int wf[NL], wl[NL];  // WIN: the frames position k * UB + lane * NL + q may own (from label_length on: never read, empty)
  if constexpr (WIN) {
    const int32_t *const wb = win + (size_t)b * wstride;
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int g = k * UB + lane * NL + q;
      wf[q] = g < L ? wb[2 * (size_t)g] : 0;
      wl[q] = g < L ? wb[2 * (size_t)g + 1] : -1;
    }
  }

  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  // vector row accesses (16 bytes of float32, 8 bytes of 16-bit elements) need aligned rows; element-wise otherwise
  const bool vec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (dt == 0 ? 15 : 7)) == 0;
  double *const row = w.row + (CKPT ? long_loss_ckpt_index(b, K, k, T, TF, j) : (size_t)b * K + k) * RW;  // row out
  const double *const row_in = CKPT && !fresh ? row - RW : row;  // (not fresh: j > 0, and tile (k, j - 1) ran)
  const double *const col_in = k > 0 ? w.col + ((size_t)b * (K - 1) + (k - 1)) * (size_t)T * 2 : nullptr;
  double *const col_out = has_right && !REDO ? w.col + ((size_t)b * (K - 1) + k) * (size_t)T * 2 : nullptr;
  [[maybe_unused]] const double *col2_in = nullptr;
  [[maybe_unused]] double *col2_out = nullptr;
  if constexpr (OPT) {
    if (k > 0) col2_in = w.col2 + ((size_t)b * (K - 1) + (k - 1)) * (size_t)T * 2;
    if (has_right && !REDO) col2_out = w.col2 + ((size_t)b * (K - 1) + k) * (size_t)T * 2;
  }
  float *const statw = w.stat + (size_t)b * T * 4;
  // the saved row of frame t_base; the rows of a tile are consecutive (without checkpoints: so are all rows of the label block)
  const int t_base = REDO ? t_lo : 0;
  double *const myrows = SAVE ? w.rows + long_loss_row_index(REDO, b, K, k, T, t_base, TF) * SRD : nullptr;

  // chain state (wave 0): row in
  double O[NL], C[NL];  // simplified: C is S, O unused
  unsigned allow = 0;   // classic: bit q = label[i] differs from label[i-1], or one of the two is a wildcard
  double cs = 0.0;      // the start state (label block 0): blank so far
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    O[q] = NINF; C[q] = NINF;
    const int i = lane * NL + q;
    if (KIND == 0 && k * UB + i > 0) {
      const int prev = lab_s[LB - 1 + i];
      if constexpr (OPT) {
        if (lab[q] != prev || ll_is_wild<true>(lab[q]) || ll_is_wild<true>(prev)) allow |= 1u << q;
      } else {
        if (lab[q] != prev || lab[q] == LONG_LOSS_WILDCARD || prev == LONG_LOSS_WILDCARD) allow |= 1u << q;
      }
    }
  }
  [[maybe_unused]] unsigned skip = 0, skipo = 0;
  if constexpr (OPT) ll_skip_bits<KIND, NL>(lab_s, k, lane * NL, skip, skipo);
  if (wave == 0 && !fresh) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      if (KIND == 0) O[q] = row_in[q * 64 + lane];
      C[q] = row_in[(NL + q) * 64 + lane];
    }
    if (k == 0) cs = row_in[2 * UB];
  }

  auto produce = [&](int kb) {  // one frame per producer wavefront
    const int f = wave - 1, t = t_lo + kb * F + f;
    if (t >= t_hi) return;
    const char *const xr = xb + (size_t)((long)t * p.xst) * esz;
    float e[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const float v = row_load1(xr, lab[q] >= 0 ? lab[q] : blank, dt);
      e[q] = lab[q] >= 0 ? v : -__builtin_inff();
    }
    float4 sv;
    if (k == 0 && !REDO) {
      // the row pass.  Both access paths give a lane the same elements in the same order: identical bits
      const float eb = row_load1(xr, blank, dt);
      float m = -3.402823466e38f, s = 0.f;
      for (int c = lane * 4; c < V; c += 256) ll_stat_add4(m, s, vec ? ll_row_load4(xr, c, dt) : ll_row_load4_elem(xr, c, V, dt));
      float M = wave_max(m);
      const float S = wave_sum(s * fexp2((m - M) * LOG2E));
      float l2s = flog2(S);
      if (!(S > 0.f)) { M = 0.f; l2s = __builtin_inff(); }  // a row of -inf: every emission of the frame is -inf
      sv = make_float4(eb, M, l2s, 0.f);
      if (lane == 0) *reinterpret_cast<float4 *>(statw + (size_t)t * 4) = sv;
    } else {
      sv = *reinterpret_cast<const float4 *>(statw + (size_t)t * 4);  // (tile (0, j) stored it on an earlier launch: the same bits)
    }
    float *const r = ring + ((kb & 1) * F + f) * RS;
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      float v = e[q];
      if constexpr (WIN) {
        if ((wild >> q) & 1u) v = 0.f;  // the gate of e_w
        if (t < wf[q] || t > wl[q]) v = -__builtin_inff();  // (t: the absolute frame, in the beta tile too)
      }
      r[lane * NL + q] = v;
    }
    if (lane == 0) *reinterpret_cast<float4 *>(r + UB) = sv;
    if (k > 0 && lane < 2) col_s[kb & 1][f][lane] = col_in[(size_t)t * 2 + lane];
    if constexpr (OPT) {
      if (k > 0 && lane >= 2 && lane < 4) col_s[kb & 1][f][lane] = col2_in[(size_t)t * 2 + lane - 2];
    }
  };

  auto consume = [&](int kb) {
    const int t0 = t_lo + kb * F;
    const int nf = t_hi - t0 < F ? t_hi - t0 : F;
    const float *const rb = ring + (kb & 1) * F * RS;
    for (int f = 0; f < nf; ++f) {
      const float *const rr = rb + f * RS;
      float e[NL];
#pragma unroll
      for (int q = 0; q < NL; ++q) e[q] = rr[lane * NL + q];
      const LlFrame fr = ll_frame_of(rr, lpin, w2);
      const double eb = fr.eb;
      auto ewq = [&](int q) { return WIN ? fr.ew + (double)e[q] : fr.ew; };  // (WIN: the ring slot of a wildcard is its gate, 0 or -inf)
      auto em = [&](int q) { return ((wild >> q) & 1u) ? ewq(q) : fma((double)e[q] - fr.Md, LOG2E_D, fr.nl2s); };
      double *const r = SAVE ? myrows + (size_t)(t0 + f - t_base) * SRD : nullptr;
      if (SAVE && KIND == 1) {  // the state BEFORE the frame
#pragma unroll
        for (int q = 0; q < NL; ++q) r[lane * NS + q] = C[q];
        if (k == 0 && lane == 0) r[SRD - 2] = cs;
      }
      if (col_out && lane == 63) {  // column out: the last position before this frame
        col_out[(size_t)(t0 + f) * 2] = O[NL - 1];
        col_out[(size_t)(t0 + f) * 2 + 1] = C[NL - 1];
      }
      if constexpr (OPT) {
        if (col2_out && lane == 63) {  // ... and the last but one
          col2_out[(size_t)(t0 + f) * 2] = O[NL - 2];
          col2_out[(size_t)(t0 + f) * 2 + 1] = C[NL - 2];
        }
      }
      const double fillO = k > 0 ? col_s[kb & 1][f][0] : NINF;
      const double fillC = k > 0 ? col_s[kb & 1][f][1] : cs;
      // OPT: the position two before the lane's first is the previous lane's last but one; before lane 0 the second column (block 0:
      // nothing lies before the start state)
      [[maybe_unused]] double fill2O = NINF, fill2C = NINF;
      if constexpr (OPT) {
        if (k > 0) { fill2O = col_s[kb & 1][f][2]; fill2C = col_s[kb & 1][f][3]; }
      }
      if (KIND == 0) {
        const double pO = from_prev_lane(O[NL - 1], fillO);
        const double pC = from_prev_lane(C[NL - 1], fillC);
        [[maybe_unused]] double pO2 = NINF, pC2 = NINF;
        if constexpr (OPT) {
          pO2 = from_prev_lane(O[NL - 2], fill2O);
          pC2 = from_prev_lane(C[NL - 2], fill2C);
        }
#pragma unroll
        for (int q = NL - 1; q >= 0; --q) {
          const double qO = q > 0 ? O[q > 0 ? q - 1 : 0] : pO;
          const double qC = q > 0 ? C[q > 0 ? q - 1 : 0] : pC;
          const double a2 = ((allow >> q) & 1u) ? qO : NINF;
          double o;
          if constexpr (OPT) {
            const double rO = q > 1 ? O[q > 1 ? q - 2 : 0] : q == 1 ? pO : pO2;
            const double rC = q > 1 ? C[q > 1 ? q - 2 : 0] : q == 1 ? pC : pC2;
            o = ll_lse(O[q], qC, a2, ((skip >> q) & 1u) ? rC : NINF, ((skipo >> q) & 1u) ? rO : NINF) + em(q);
          } else {
            o = ll_lse(O[q], qC, a2) + em(q);
          }
          C[q] = ll_lse(C[q], O[q]) + eb;
          O[q] = o;
        }
      } else {
        const double pS = from_prev_lane(C[NL - 1], fillC);
        [[maybe_unused]] double pS2 = NINF;
        if constexpr (OPT) pS2 = from_prev_lane(C[NL - 2], fill2C);
#pragma unroll
        for (int q = NL - 1; q >= 0; --q) {
          const double s = q > 0 ? C[q > 0 ? q - 1 : 0] : pS;
          if constexpr (OPT) {
            const double r = q > 1 ? C[q > 1 ? q - 2 : 0] : q == 1 ? pS : pS2;
            C[q] = ll_lse(C[q] + (((wild >> q) & 1u) ? ewq(q) : eb), s + em(q), ((skip >> q) & 1u) ? r + em(q) : NINF);
          } else {
            C[q] = ll_lse(C[q] + (((wild >> q) & 1u) ? ewq(q) : eb), s + em(q));
          }
        }
      }
      cs += eb;
      if (SAVE && KIND == 0) {  // the state AFTER the frame
#pragma unroll
        for (int q = 0; q < NL; ++q) *reinterpret_cast<double2 *>(r + lane * NS + 2 * q) = make_double2(O[q], C[q]);
        if (k == 0 && lane == 0) r[SRD - 2] = cs;
      }
    }
  };

  const int nb = (t_hi - t_lo + F - 1) / F;
  if (wave > 0) produce(0);
  __syncthreads();
  for (int kb = 0; kb < nb; ++kb) {
    if (wave == 0) consume(kb);
    else if (kb + 1 < nb) produce(kb + 1);
    __syncthreads();
  }

  // row out
  if (wave == 0 && !REDO) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      row[q * 64 + lane] = O[q];
      row[(NL + q) * 64 + lane] = C[q];
    }
    if (k == 0 && lane == 0) row[2 * UB] = cs;
  }
}

// log2 Z of every utterance from the row buffers: one thread per utterance.  CKPT: from the checkpoint that the block's last tile
// in time, (k, (Tb - 1) / TF), wrote (it ran: 0 < L <= Tb, or block 0 of an empty transcript with Tb > 0)
// OPT: behind an optional last position, position L - 2 (L = 1: the start state) ends the utterance too; it may live in the block
// before.  A block none of whose tiles ran (its positions lie beyond what the frames reach) holds log 0; TF: always given
template <int KIND, bool CKPT, bool OPT>
__device__ __forceinline__ void loss_long_finish(const Problem &p, const LongLossWs &w, int K, int TF, float *__restrict__ loss) {
  const double NINF = -__builtin_inf();
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= p.B) return;
  const int Tb = frame_count(p, b);
  const int L = label_count(p, b);
  auto row_of = [&](int k) { return w.row + (CKPT ? long_loss_ckpt_index(b, K, k, p.T, TF, (Tb - 1) / TF) : (size_t)b * K + k) * RW; };
  double v = NINF;
  if constexpr (OPT) {
    const bool last_opt = !too_many_labels(p, L) && ll_last_optional(p, b, L);
    // the state of position i behind the last frame: log 0 where the block's last tile in time did not run (then none of it did)
    auto end_of = [&](int i) {
      const int kk = i / UB, r = i % UB;
      if (!long_loss_tile_active_opt(Tb, L, kk, (Tb - 1) / TF, TF)) return NINF;
      const double *const row = row_of(kk);
      const double ov = row[(r % NL) * 64 + r / NL], cv = row[(NL + r % NL) * 64 + r / NL];
      return KIND == 0 ? ll_lse(ov, cv) : cv;
    };
    if (too_many_labels(p, L) || L / 2 > Tb) {
      // infeasible by the count: no tile ran
    } else if (Tb == 0) {  // (L <= 1) no frame: the empty path, if the transcript allows it
      v = L == 0 || last_opt ? 0.0 : NINF;
    } else if (L == 0) {
      v = row_of(0)[2 * UB];
    } else {
      v = end_of(L - 1);
      if (last_opt) v = ll_lse(v, L == 1 ? row_of(0)[2 * UB] : end_of(L - 2));
    }
  } else if (too_many_labels(p, L) || L > Tb) {
    // infeasible by the count: no tile ran
  } else if (L == 0) {
    v = Tb == 0 ? 0.0 : row_of(0)[2 * UB];
  } else {  // (L <= Tb: block (L - 1) / UB ran at least one tile)
    const int i = L - 1, r = i % UB;
    const double *const row = row_of(i / UB);
    const double ov = row[(r % NL) * 64 + r / NL], cv = row[(NL + r % NL) * 64 + r / NL];
    v = KIND == 0 ? ll_lse(ov, cv) : cv;
  }
  loss[b] = (float)(0.0 - v * LN2_D);  // (-inf: +inf; an empty utterance: +0)
  w.logp[b] = v;
  w.flag[b] = v > NINF && v < -NINF ? 1 : 0;
}
template <int KIND>
__global__ __launch_bounds__(256) void loss_long_finish_kernel(const Problem p, const LongLossWs w, int K, float *__restrict__ loss) {
  loss_long_finish<KIND, false, false>(p, w, K, 0, loss);
}
template <int KIND>
__global__ __launch_bounds__(256) void loss_long_finish_ckpt_kernel(const Problem p, const LongLossWs w, int K, int TF,
                                                                    float *__restrict__ loss) {
  loss_long_finish<KIND, true, false>(p, w, K, TF, loss);
}
template <int KIND, bool CKPT>
__global__ __launch_bounds__(256) void loss_long_finish_opt_kernel(const Problem p, const LongLossWs w, int K, int TF,
                                                                   float *__restrict__ loss) {
  loss_long_finish<KIND, CKPT, true>(p, w, K, TF, loss);
}

// CKPT: the saved rows are the ring's (long_loss_row_index), written by alpha MODE 3 on the launch before this one
template <int KIND, bool CKPT, bool WIN, bool OPT>
__global__ __launch_bounds__(LL_THREADS) void loss_long_beta_kernel(const Problem p, const double w2, const LlWsArg<OPT> w, int K, int TF,
                                                                    int d, int k_lo, int count, const int32_t *__restrict__ win,
                                                                    int wstride) {
  constexpr int NS = (KIND == 0 ? 2 : 1) * NL;
  constexpr int SRD = long_loss_row_doubles(KIND);
  static_assert(!(WIN && OPT), "frame windows and optional wildcards are not combined");
  constexpr int LB = OPT ? 2 : 1;  // lab_s[LB + i]: position k * UB + i
  const double NINF = -__builtin_inf();
  __shared__ __attribute__((aligned(16))) float ring[2 * F * RS];
  __shared__ int lab_s[UB + 2 * LB];  // positions k * UB - LB .. k * UB + UB + LB - 1
  // [0]: the worth of entering position (k + 1) * UB with the frame; [1]: simplified, alpha of k * UB - 1 before it; OPT: [2], [3]
  // the same of positions (k + 1) * UB + 1 and k * UB - 2
  __shared__ double col_s[2][F][2 * LB];

  const int b = blockIdx.x / count, k = k_lo + blockIdx.x % count, j = d - k;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = p.T, blank = p.blank, dt = p.xdtype;
  const bool lpin = p.wrt != 0;
  const int Tb = frame_count(p, b);
  const int L = label_count(p, b);
  // an infeasible utterance has no posteriors: the row stage writes its zeros without them
  if (too_many_labels(p, L) || !ll_tile_active<OPT>(Tb, L, k, j, TF) || w.flag[b] == 0) return;
  const double lP = w.logp[b];
  const int t_lo = j * TF;
  const int t_hi = Tb - t_lo < TF ? Tb : t_lo + TF;
  const bool fresh = long_loss_beta_fresh(Tb, j, TF);
  const bool right = OPT ? long_loss_beta_has_right_opt(Tb, L, k, j, TF) : long_loss_beta_has_right(Tb, L, k, j, TF);

  if constexpr (OPT) ll_labels_opt(p, b, k, L, UB + 2 * LB, lab_s);
  else ll_labels(p, b, k, L, UB + 2 * LB, lab_s);
  __syncthreads();

  int lab[NL];
  unsigned wild = 0;
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    lab[q] = lab_s[LB + lane * NL + q];
    if constexpr (OPT) {
      if (ll_is_wild<true>(lab[q])) wild |= 1u << q;
    } else {
      if (lab[q] == LONG_LOSS_WILDCARD) wild |= 1u << q;
    }
  }
  [[maybe_unused]] int wf[NL], wl[NL];  // WIN: the frames position k * UB + lane * NL + q may own (from label_length on: never read, empty)
  if constexpr (WIN) {
    const int32_t *const wb = win + (size_t)b * wstride;
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int g = k * UB + lane * NL + q;
      wf[q] = g < L ? wb[2 * (size_t)g] : 0;
      wl[q] = g < L ? wb[2 * (size_t)g + 1] : -1;
    }
  }

  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  double *const row = w.rowb + ((size_t)b * K + k) * RW;
  const double *const colb_in = right ? w.colb + ((size_t)b * (K - 1) + k) * (size_t)T : nullptr;
  double *const colb_out = k > 0 ? w.colb + ((size_t)b * (K - 1) + (k - 1)) * (size_t)T : nullptr;
  const double *const cola_in = KIND == 1 && k > 0 ? w.col + ((size_t)b * (K - 1) + (k - 1)) * (size_t)T * 2 : nullptr;
  [[maybe_unused]] const double *colb2_in = nullptr, *cola2_in = nullptr;
  [[maybe_unused]] double *colb2_out = nullptr;
  if constexpr (OPT) {
    if (right) colb2_in = w.colb2 + ((size_t)b * (K - 1) + k) * (size_t)T;
    if (k > 0) colb2_out = w.colb2 + ((size_t)b * (K - 1) + (k - 1)) * (size_t)T;
    if (KIND == 1 && k > 0) cola2_in = w.col2 + ((size_t)b * (K - 1) + (k - 1)) * (size_t)T * 2;
  }
  const float *const statw = w.stat + (size_t)b * T * 4;
  // the saved row of frame t_base; the rows of a tile are consecutive (without checkpoints: so are all rows of the label block)
  const int t_base = CKPT ? t_lo : 0;
  double *const myrows = w.rows + long_loss_row_index(CKPT, b, K, k, T, t_base, TF) * SRD;

  // chain state (wave 0): beta, the mass of the frames still to come
  double O[NL], C[NL];
  unsigned allow = 0;
  int allow_nx = 0;  // ... of the next lane's first position (lane 63: position (k + 1) * UB)
  double cs = NINF;
  auto allowed = [&](int i) {  // position k * UB + i, 0 <= i <= UB
    if (k * UB + i <= 0) return false;
    const int a = lab_s[LB + i], q = lab_s[LB - 1 + i];
    if constexpr (OPT) return a != q || ll_is_wild<true>(a) || ll_is_wild<true>(q);
    else return a != q || a == LONG_LOSS_WILDCARD || q == LONG_LOSS_WILDCARD;
  };
#pragma unroll
  for (int q = 0; q < NL; ++q)
    if (KIND == 0 && allowed(lane * NL + q)) allow |= 1u << q;
  if (KIND == 0) allow_nx = allowed((lane + 1) * NL) ? 1 : 0;
  // OPT: the skip bits of the lane's positions and the two behind them (the sweep looks two ahead; lane 63: into the next block)
  [[maybe_unused]] unsigned skip = 0, skipo = 0;
  [[maybe_unused]] bool last_opt = false;
  if constexpr (OPT) {
    ll_skip_bits<KIND, NL + 2>(lab_s, k, lane * NL, skip, skipo);
    last_opt = ll_last_optional(p, b, L);
  }
  if (fresh) {  // behind the last frame only the end states have any mass
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const int g = k * UB + lane * NL + q;
      O[q] = C[q] = (g == L - 1 || (OPT && last_opt && g == L - 2)) ? 0.0 : NINF;
    }
    if (k == 0 && (L == 0 || (OPT && last_opt && L == 1))) cs = 0.0;
  } else {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      O[q] = row[q * 64 + lane];
      C[q] = row[(NL + q) * 64 + lane];
    }
    if (k == 0) cs = row[2 * UB];
  }

  // ring position q of the tile stands for frame t_hi - 1 - q
  auto produce = [&](int kb) {
    const int f = wave - 1, t = t_hi - 1 - (kb * F + f);
    if (t < t_lo) return;
    const char *const xr = xb + (size_t)((long)t * p.xst) * esz;
    float e[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      const float v = row_load1(xr, lab[q] >= 0 ? lab[q] : blank, dt);
      e[q] = lab[q] >= 0 ? v : -__builtin_inff();
    }
    float *const r = ring + ((kb & 1) * F + f) * RS;
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      float v = e[q];
      if constexpr (WIN) {
        if ((wild >> q) & 1u) v = 0.f;  // the gate of e_w
        if (t < wf[q] || t > wl[q]) v = -__builtin_inff();  // (t: the absolute frame, in the beta tile too)
      }
      r[lane * NL + q] = v;
    }
    if (lane == 0) {
      *reinterpret_cast<float4 *>(r + UB) = *reinterpret_cast<const float4 *>(statw + (size_t)t * 4);  // (the alpha sweep stored it)
      col_s[kb & 1][f][0] = colb_in ? colb_in[t] : NINF;
    } else if (lane == 1) {
      col_s[kb & 1][f][1] = cola_in ? cola_in[(size_t)t * 2 + 1] : NINF;
    }
    if constexpr (OPT) {
      if (lane == 2) col_s[kb & 1][f][2] = colb2_in ? colb2_in[t] : NINF;
      else if (lane == 3) col_s[kb & 1][f][3] = cola2_in ? cola2_in[(size_t)t * 2 + 1] : NINF;
    }
  };

  auto consume = [&](int kb) {
    const int q0 = kb * F;
    const int nf = t_hi - t_lo - q0 < F ? t_hi - t_lo - q0 : F;
    const float *const rb = ring + (kb & 1) * F * RS;
    for (int f = 0; f < nf; ++f) {
      const int t = t_hi - 1 - (q0 + f);
      const float *const rr = rb + f * RS;
      float e[NL];
#pragma unroll
      for (int q = 0; q < NL; ++q) e[q] = rr[lane * NL + q];
      const LlFrame fr = ll_frame_of(rr, lpin, w2);
      const double eb = fr.eb;
      auto ewq = [&](int q) { return WIN ? fr.ew + (double)e[q] : fr.ew; };  // (WIN: the ring slot of a wildcard is its gate, 0 or -inf)
      auto em = [&](int q) { return ((wild >> q) & 1u) ? ewq(q) : fma((double)e[q] - fr.Md, LOG2E_D, fr.nl2s); };
      double *const r = myrows + (size_t)(t - t_base) * SRD;
      double A[NS], Acs = NINF;
#pragma unroll
      for (int q = 0; q < NS; ++q) A[q] = r[lane * NS + q];
      if (k == 0) Acs = r[SRD - 2];
      const double fillR = col_s[kb & 1][f][0];
      auto post = [&](double l2) { return fexp2((float)(l2 - lP)); };
      if (KIND == 0) {
#pragma unroll
        for (int q = 0; q < NL; ++q)
          *reinterpret_cast<float2 *>(r + lane * NS + 2 * q) = make_float2(post(A[2 * q] + O[q]), post(A[2 * q + 1] + C[q]));
        if (k == 0 && lane == 0) *reinterpret_cast<float *>(r + SRD - 2) = post(Acs + cs);
        // beta back over frame t: x = what entering O[i] with this frame is worth
        double x = O[0] + em(0);
        if (colb_out && lane == 0) colb_out[t] = x;
        const double xl = from_next_lane(x, fillR);
        if constexpr (OPT) {
          // the mirror image of the alpha step: what entering the open states one and two positions ahead is worth; beyond the
          // lane's own they are the next lane's first two, beyond lane 63 the two beta columns
          double x1 = O[1] + em(1);
          if (colb2_out && lane == 0) colb2_out[t] = x1;
          const double xl2 = from_next_lane(x1, col_s[kb & 1][f][2]);
          cs = ll_lse(cs + eb, x, ((skip >> 1) & 1u) ? x1 : NINF);
#pragma unroll
          for (int q = 0; q < NL; ++q) {
            const double x2 = q + 2 < NL ? O[q + 2 < NL ? q + 2 : 0] + em(q + 2 < NL ? q + 2 : 0) : q + 2 == NL ? xl : xl2;
            const bool al = q + 1 < NL ? ((allow >> (q + 1)) & 1u) != 0 : allow_nx != 0;
            const double cb = C[q] + eb;
            O[q] = ll_lse(x, cb, al ? x1 : NINF, ((skipo >> (q + 2)) & 1u) ? x2 : NINF);
            C[q] = ll_lse(cb, x1, ((skip >> (q + 2)) & 1u) ? x2 : NINF);
            x = x1;
            x1 = x2;
          }
        } else {
          cs = ll_lse(cs + eb, x);
#pragma unroll
          for (int q = 0; q < NL; ++q) {
            const double xn = q + 1 < NL ? O[q + 1 < NL ? q + 1 : 0] + em(q + 1 < NL ? q + 1 : 0) : xl;
            const bool al = q + 1 < NL ? ((allow >> (q + 1)) & 1u) != 0 : allow_nx != 0;
            const double cb = C[q] + eb;
            O[q] = ll_lse(x, cb, al ? xn : NINF);
            C[q] = ll_lse(cb, xn);
            x = xn;
          }
        }
      } else {
        const double ap0 = from_prev_lane(A[NL - 1], k > 0 ? col_s[kb & 1][f][1] : Acs);
        [[maybe_unused]] double ap00 = NINF;  // OPT: alpha two positions before the lane's first (block 0: nothing before the start state)
        if constexpr (OPT) ap00 = from_prev_lane(A[NL - 2], k > 0 ? col_s[kb & 1][f][3] : NINF);
#pragma unroll
        for (int q = 0; q < NL; ++q) {
          double ap = q > 0 ? A[q > 0 ? q - 1 : 0] : ap0;
          if constexpr (OPT) {  // entered from one position back or, over an optional wildcard, from two
            const double ap2 = q > 1 ? A[q > 1 ? q - 2 : 0] : q == 1 ? ap0 : ap00;
            ap = ll_lse(ap, ((skip >> q) & 1u) ? ap2 : NINF);
          }
          const double h = ((wild >> q) & 1u) ? ewq(q) : eb;
          *reinterpret_cast<float2 *>(r + lane * NS + q) = make_float2(post(ap + em(q) + C[q]), post(A[q] + h + C[q]));
        }
        if (k == 0 && lane == 0) *reinterpret_cast<float *>(r + SRD - 2) = post(Acs + eb + cs);
        double x = C[0] + em(0);
        if (colb_out && lane == 0) colb_out[t] = x;
        const double xl = from_next_lane(x, fillR);
        if constexpr (OPT) {
          double x1 = C[1] + em(1);
          if (colb2_out && lane == 0) colb2_out[t] = x1;
          const double xl2 = from_next_lane(x1, col_s[kb & 1][f][2]);
          cs = ll_lse(cs + eb, x, ((skip >> 1) & 1u) ? x1 : NINF);
#pragma unroll
          for (int q = 0; q < NL; ++q) {
            const double x2 = q + 2 < NL ? C[q + 2 < NL ? q + 2 : 0] + em(q + 2 < NL ? q + 2 : 0) : q + 2 == NL ? xl : xl2;
            C[q] = ll_lse(C[q] + (((wild >> q) & 1u) ? ewq(q) : eb), x1, ((skip >> (q + 2)) & 1u) ? x2 : NINF);
            x1 = x2;
          }
        } else {
          cs = ll_lse(cs + eb, x);
#pragma unroll
          for (int q = 0; q < NL; ++q) {
            const double xn = q + 1 < NL ? C[q + 1 < NL ? q + 1 : 0] + em(q + 1 < NL ? q + 1 : 0) : xl;
            C[q] = ll_lse(C[q] + (((wild >> q) & 1u) ? ewq(q) : eb), xn);
            x = xn;
          }
        }
      }
    }
  };

  const int nb = (t_hi - t_lo + F - 1) / F;
  if (wave > 0) produce(0);
  __syncthreads();
  for (int kb = 0; kb < nb; ++kb) {
    if (wave == 0) consume(kb);
    else if (kb + 1 < nb) produce(kb + 1);
    __syncthreads();
  }

  // row out: beta before the tile's first frame, for the tile before it in time
  if (wave == 0) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      row[q * 64 + lane] = O[q];
      row[(NL + q) * 64 + lane] = C[q];
    }
    if (k == 0 && lane == 0) row[2 * UB] = cs;
  }
}

// ---- the gradient's row stage: one wavefront per row (b, t), four per workgroup ----
constexpr int LLG_WAVES = 4;
constexpr int LLG_CH = 1024;  // columns per pass
constexpr int LLG_FIX = 40;   // fixed point: a posterior (in [0, 1]) in units of 2^-40, so |bin| < U 2^40 <= 2^56

// CKPT: the rows (b, t) of one time block, t = t0 .. t0 + nt - 1, from the ring; otherwise all of them (t0 = 0, nt = T)
// OPT: an optional wildcard counts as a wildcard (a feasible utterance has no bad pair), and the tiles are those of the optional predicate
template <int KIND, bool CKPT, bool OPT>
__device__ __forceinline__ void loss_long_row(const Problem &p, const LongLossWs &w, int K, int TF, int t0, int nt,
                                              const float *__restrict__ d_loss, void *__restrict__ grad) {
  constexpr int SLOT = KIND == 0 ? 16 : 8;  // bytes of a label position in a saved row; its first 8 are the two posteriors
  constexpr size_t ROWB = (size_t)long_loss_row_doubles(KIND) * 8;
  __shared__ unsigned long long bins_all[LLG_WAVES][LLG_CH];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long rowi = (long)blockIdx.x * LLG_WAVES + wv;
  if (rowi >= (long)p.B * nt) return;  // (wavefront-uniform; nothing below synchronises beyond the wavefront)
  unsigned long long *const bins = bins_all[wv];
  const int b = (int)(rowi / nt), t = t0 + (int)(rowi % nt);
  const int V = p.V, blank = p.blank, xdt = p.xdtype, gdt = p.gdtype;
  const int Tb = frame_count(p, b);
  const int xesz = xdt == 0 ? 4 : 2, gesz = gdt == 0 ? 4 : 2;
  const char *const x = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb + (long)t * p.xst) * xesz;
  char *const g = reinterpret_cast<char *>(grad) + (size_t)((long)b * p.gsb + (long)t * p.gst) * gesz;
  const bool xvec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (xdt == 0 ? 15 : 7)) == 0;
  const bool gvec = ((V | p.gsb | p.gst) & 3) == 0 && (reinterpret_cast<uintptr_t>(grad) & (gdt == 0 ? 15 : 7)) == 0;

  // four consecutive elements of the gradient row from column c (c + 3 < V on the vector path; both paths convert alike)
  auto gput4 = [&](int c, const float4 r) {
    if (gdt == 0) {
      if (gvec) { *reinterpret_cast<float4 *>(g + (size_t)c * 4) = r; return; }
      float *const o = reinterpret_cast<float *>(g);
      o[c] = r.x;
      if (c + 1 < V) o[c + 1] = r.y;
      if (c + 2 < V) o[c + 2] = r.z;
      if (c + 3 < V) o[c + 3] = r.w;
      return;
    }
    auto cv = [&](float f) { return gdt == 1 ? f32_to_bf16(f) : f32_to_f16(f); };
    const unsigned short h0 = cv(r.x), h1 = cv(r.y), h2 = cv(r.z), h3 = cv(r.w);
    if (gvec) {
      *reinterpret_cast<uint2 *>(g + (size_t)c * 2) = make_uint2((unsigned)h0 | ((unsigned)h1 << 16), (unsigned)h2 | ((unsigned)h3 << 16));
      return;
    }
    unsigned short *const o = reinterpret_cast<unsigned short *>(g);
    o[c] = h0;
    if (c + 1 < V) o[c + 1] = h1;
    if (c + 2 < V) o[c + 2] = h2;
    if (c + 3 < V) o[c + 3] = h3;
  };

  // an infinite loss contributes nothing and its d_loss is not interpreted
  if (!(t < Tb) || w.flag[b] == 0) {  // a padded frame, an infeasible utterance: exactly zero
    for (int c = lane * 4; c < V; c += 256) gput4(c, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  const float dl = d_loss ? d_loss[b] : 1.f;
  if constexpr (OPT) {  // a weight of zero: +0 throughout, as above (0 * a negative element would be -0)
    if (dl == 0.f) {
      for (int c = lane * 4; c < V; c += 256) gput4(c, make_float4(0.f, 0.f, 0.f, 0.f));
      return;
    }
  }
  const float4 sv = *reinterpret_cast<const float4 *>(w.stat + ((size_t)b * p.T + t) * 4);
  const float mx = sv.y, l2s = sv.z;
  const int L = label_count(p, b);  // (feasible: L <= U)
  const int j = t / TF;
  // the saved row of (b, 0, t); those of the other label blocks lie long_loss_row_stride rows apart
  const char *const rows = reinterpret_cast<const char *>(w.rows) + long_loss_row_index(CKPT, b, K, 0, p.T, t, TF) * ROWB;
  const size_t kstride = long_loss_row_stride(CKPT, K, p.T, TF);
  const int32_t *const lab = label_row(p, b);

  float blk = 0.f, gam = 0.f;  // the blank's share and Gamma_t, lane-wise partial sums in a fixed order
  for (int c0 = 0; c0 < V; c0 += LLG_CH) {
#pragma unroll
    for (int q = 0; q < LLG_CH / 64; ++q) bins[lane + 64 * q] = 0ull;
    wave_lds_fence();
    for (int k = 0; k < K && (k == 0 || k * UB < L); ++k) {
      // a tile that did not run has no posteriors: they are exactly zero, and adding them would change no bit
      if (!ll_tile_active<OPT>(Tb, L, k, j, TF)) continue;
      const char *const r = rows + (size_t)k * kstride * ROWB;
      const int n = L - k * UB < UB ? L - k * UB : UB;
      for (int i = lane; i < n; i += 64) {
        const float2 pq = *reinterpret_cast<const float2 *>(r + (size_t)i * SLOT);
        const int tok = label_at(p, lab, k * UB + i);
        const bool wc = ll_is_wild<OPT>(tok);
        const unsigned rel = (unsigned)(tok - c0);
        if (!wc && emits(p, tok) && rel < (unsigned)LLG_CH)
          atomicAdd(&bins[rel], (unsigned long long)__float2ll_rn(__builtin_ldexpf(pq.x, LLG_FIX)));
        if (c0 == 0) {
          if (wc) gam += pq.x;
          if (KIND == 1 && wc) gam += pq.y;
          else blk += pq.y;
        }
      }
      if (c0 == 0 && k == 0 && lane == 0) blk += *reinterpret_cast<const float *>(r + (size_t)UB * SLOT);  // the start state
    }
    if (c0 == 0) {
      blk = wave_sum(blk);
      gam = wave_sum(gam);
    }
    wave_lds_fence();
    // logits: (1 - Gamma) softmax - gamma;  log-probabilities: -Gamma exp(x - LSE) - gamma
    const float c = p.wrt == 0 ? 1.f - gam : -gam;
#pragma unroll
    for (int q = 0; q < LLG_CH / 256; ++q) {
      const int col = c0 + lane * 4 + 256 * q;
      if (col < V) {
        const float4 xv = xvec ? ll_row_load4(x, col, xdt) : ll_row_load4_elem(x, col, V, xdt);
        float o[4];
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          const float bin = __builtin_ldexpf(__ll2float_rn((long long)bins[col - c0 + cc]), -LLG_FIX) + (col + cc == blank ? blk : 0.f);
          const float sm = c == 0.f ? 0.f : c * fexp2((xs[cc] - mx) * LOG2E - l2s);
          o[cc] = dl * (sm - bin);
        }
        gput4(col, make_float4(o[0], o[1], o[2], o[3]));
      }
    }
    wave_lds_fence();
  }
}
template <int KIND, bool OPT>
__global__ __launch_bounds__(64 * LLG_WAVES) void loss_long_row_kernel(const Problem p, const LongLossWs w, int K, int TF,
                                                                       const float *__restrict__ d_loss, void *__restrict__ grad) {
  loss_long_row<KIND, false, OPT>(p, w, K, TF, 0, p.T, d_loss, grad);
}
template <int KIND, bool OPT>
__global__ __launch_bounds__(64 * LLG_WAVES) void loss_long_row_ckpt_kernel(const Problem p, const LongLossWs w, int K, int TF, int t0, int nt,
                                                                            const float *__restrict__ d_loss, void *__restrict__ grad) {
  loss_long_row<KIND, true, OPT>(p, w, K, TF, t0, nt, d_loss, grad);
}

// ---- the posterior stage of ctc_amd_long_label_posterior: the ring rows of one time block, read a second
// way.  One launch, two kinds of wavefront, LONG_POST_WAVES to a workgroup; neither waits for the other, both only read the ring ----
struct LongPostOut {
  float *post, *blk;       // label_posterior [B][T][U] (nullptr: not wanted), blank_posterior [B][T]
  float *dur, *exf, *peak; // [B][U] each; dur and exf both or neither, peak and peak_frame both or neither
  int *peak_frame;
  double2 *acc;            // workspace, [B][U]: (sum p, sum t p) over the frames met so far, descending
  float2 *pk;              // workspace, [B][U]: the running peak and (as an int's bits) its frame
};

// what a position's slot of a ring row says: the value label_posterior[b, t, i] takes
template <int KIND>
__device__ __forceinline__ float ll_post_value(const float2 pq, bool wc) {
  return KIND == 1 && wc ? pq.x + pq.y : pq.x;
}

// Workgroups 0 .. row_groups - 1, one wavefront per row (b, t) of time block d (t = d * TF .. d * TF + nt - 1): the dense run of U
// floats (when wanted) and blank_posterior[b, t], the blank's share summed in the row stage's order.  The workgroups behind them,
// one wavefront per (b, 64 positions), a lane a position: the block's frames downwards into (sum p, sum t p, peak, its frame),
// carried in the workspace from the stage of time block J - 1 (`first`: starts from nothing) to that of block 0 (`last`: rounds and
// writes the four [B][U] outputs).  nt == 0 (T == 0): nothing but that.
template <int KIND, bool OPT>
__global__ __launch_bounds__(64 * LONG_POST_WAVES) void loss_long_post_kernel(const Problem p, const LongLossWs w, const LongPostOut o, int K, int TF,
                                                                              int d, int nt, unsigned row_groups, int first, int last) {
  constexpr int SLOT = KIND == 0 ? 16 : 8;  // bytes of a label position in a saved row; its first 8 are the two posteriors
  constexpr size_t ROWB = (size_t)long_loss_row_doubles(KIND) * 8;
  __shared__ __attribute__((aligned(16))) float stage_all[LONG_POST_WAVES][UB];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int U = p.U, t0 = d * TF;
  const size_t kstride = long_loss_row_stride(1, K, p.T, TF);

  if (blockIdx.x < row_groups) {
    const long rowi = (long)blockIdx.x * LONG_POST_WAVES + wv;
    if (rowi >= (long)p.B * nt) return;  // (wavefront-uniform; nothing below synchronises beyond the wavefront)
    float *const st = stage_all[wv];
    const int b = (int)(rowi / nt), t = t0 + (int)(rowi % nt);
    const int Tb = frame_count(p, b);
    const int L = label_count(p, b);
    const bool live = t < Tb && w.flag[b] != 0;  // (feasible: L <= U)
    float *const out = o.post ? o.post + ((size_t)b * p.T + t) * (size_t)U : nullptr;
    const bool vec = (U & 3) == 0 && (reinterpret_cast<uintptr_t>(o.post) & 15) == 0;
    const char *const rows = reinterpret_cast<const char *>(w.rows) + long_loss_row_index(1, b, K, 0, p.T, t, TF) * ROWB;
    const int32_t *const lab = label_row(p, b);
    float blk = 0.f;  // the blank's share, lane-wise partial sums in a fixed order
    for (int k = 0; k < K; ++k) {
      const int u0 = k * UB;
      const int nu = U - u0 < UB ? U - u0 : UB;  // positions of the block that have a column
      // a padded frame, an infeasible utterance, a block beyond the labels, a tile that did not run: exactly zero
      int n = 0;
      const bool ran = live && (k == 0 || u0 < L) && ll_tile_active<OPT>(Tb, L, k, d, TF);
      if (ran) n = L - u0 < UB ? L - u0 : UB;
      const char *const r = rows + (size_t)k * kstride * ROWB;
      for (int i = lane; i < n; i += 64) {
        const float2 pq = *reinterpret_cast<const float2 *>(r + (size_t)i * SLOT);
        const bool wc = ll_is_wild<OPT>(label_at(p, lab, u0 + i));
        if (!(KIND == 1 && wc)) blk += pq.y;
        if (out) st[i] = ll_post_value<KIND>(pq, wc);
      }
      if (ran && k == 0 && lane == 0) blk += *reinterpret_cast<const float *>(r + (size_t)UB * SLOT);  // the start state
      if (out) {
        wave_lds_fence();
        if (vec) {  // (U and u0 multiples of 4: so is nu)
          for (int c = lane * 4; c < nu; c += 256) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c + 3 < n) {
              v = *reinterpret_cast<const float4 *>(st + c);
            } else if (c < n) {
              v.x = st[c];
              if (c + 1 < n) v.y = st[c + 1];
              if (c + 2 < n) v.z = st[c + 2];
            }
            *reinterpret_cast<float4 *>(out + u0 + c) = v;
          }
        } else {
          for (int i = lane; i < nu; i += 64) out[u0 + i] = i < n ? st[i] : 0.f;
        }
        wave_lds_fence();
      }
    }
    blk = wave_sum(blk);
    if (lane == 0) o.blk[(size_t)b * p.T + t] = blk;
    return;
  }

  // the per-position statistics
  const int groups = (U + 63) / 64;
  const long wi = (long)(blockIdx.x - row_groups) * LONG_POST_WAVES + wv;
  if (wi >= (long)p.B * groups) return;
  const int b = (int)(wi / groups), i = (int)(wi % groups) * 64 + lane;
  if (i >= U) return;
  const int Tb = frame_count(p, b);
  const int L = label_count(p, b);
  const bool mine = w.flag[b] != 0 && i < L;  // (feasible: L <= U)
  const size_t at = (size_t)b * U + i;
  const bool stats = o.dur != nullptr, peaks = o.peak != nullptr;
  double sd = 0.0, sm = 0.0;
  float pk = -1.f;  // (below every posterior)
  int pf = -1;
  if (!first) {
    if (stats) { const double2 a = o.acc[at]; sd = a.x; sm = a.y; }
    if (peaks) { const float2 q = o.pk[at]; pk = q.x; pf = __float_as_int(q.y); }
  }
  const int k = i / UB;
  // (a tile that did not run: its posteriors are exactly zero; the sums keep their bits, and a peak of zero is settled below)
  if (mine && nt > 0 && ll_tile_active<OPT>(Tb, L, k, d, TF)) {
    const bool wc = ll_is_wild<OPT>(label_at(p, label_row(p, b), i));
    const int t_hi = Tb - t0 < nt ? Tb : t0 + nt;  // one past the block's last frame of this utterance (> t0: the tile runs)
    const char *const r = reinterpret_cast<const char *>(w.rows) + long_loss_row_index(1, b, K, k, p.T, t0, TF) * ROWB + (size_t)(i - k * UB) * SLOT;
    auto take = [&](int t, const float2 pq) {  // strictly in descending frame order
      const float v = ll_post_value<KIND>(pq, wc);
      sd += (double)v;
      sm += (double)t * (double)v;  // (exact in float64: fused or not, the same bits)
      if (v >= pk) { pk = v; pf = t; }  // (descending: the lowest frame that attains the peak stays)
    };
    int t = t_hi - 1;
    for (; t - 7 >= t0; t -= 8) {  // eight loads in flight, the adds in order
      float2 q[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) q[u] = *reinterpret_cast<const float2 *>(r + (size_t)(t - u - t0) * ROWB);
#pragma unroll
      for (int u = 0; u < 8; ++u) take(t - u, q[u]);
    }
    for (; t >= t0; --t) take(t, *reinterpret_cast<const float2 *>(r + (size_t)(t - t0) * ROWB));
  }
  if (!last) {
    if (stats) o.acc[at] = make_double2(sd, sm);
    if (peaks) o.pk[at] = make_float2(pk, __int_as_float(pf));
    return;
  }
  if (stats) {
    o.dur[at] = mine ? (float)sd : 0.f;
    o.exf[at] = mine && sd > 0.0 ? (float)(sm / sd) : -1.f;
  }
  if (peaks) {
    // every posterior of a position zero (or none above it in a tile that ran): the peak is 0, first attained at frame 0
    if (mine && !(pk > 0.f)) { pk = 0.f; pf = Tb > 0 ? 0 : -1; }
    o.peak[at] = mine ? pk : 0.f;
    o.peak_frame[at] = mine ? pf : -1;
  }
}

// the window of a call: nullptr runs the WIN = false kernels; optional: the OPT kernels (never with a window)
struct LlWindow {
  const int32_t *win;
  int stride;
  bool optional;
};

template <int KIND, int MODE>
void launch_alpha(const Problem &p, const LongLossPlan &P, double w2, const LongLossWsOpt &wo, const LlWindow &fw, int d, int k_lo, int count,
                  hipStream_t st) {
  if (fw.optional) {
    hipLaunchKernelGGL((loss_long_alpha_kernel<KIND, MODE, false, true>), dim3((unsigned)((size_t)p.B * count)), dim3(LL_THREADS), 0, st, p, w2,
                       wo, P.K, P.TF, d, k_lo, count, fw.win, fw.stride);
    return;
  }
  const LongLossWs &w = wo;
  const auto tile = fw.win ? loss_long_alpha_kernel<KIND, MODE, true, false> : loss_long_alpha_kernel<KIND, MODE, false, false>;
  hipLaunchKernelGGL(tile, dim3((unsigned)((size_t)p.B * count)), dim3(LL_THREADS), 0, st, p, w2, w, P.K, P.TF, d, k_lo, count, fw.win, fw.stride);
}
template <int KIND, bool CKPT>
void launch_beta(const Problem &p, const LongLossPlan &P, double w2, const LongLossWsOpt &wo, const LlWindow &fw, int d, int k_lo, int count,
                 hipStream_t st) {
  if (fw.optional) {
    hipLaunchKernelGGL((loss_long_beta_kernel<KIND, CKPT, false, true>), dim3((unsigned)((size_t)p.B * count)), dim3(LL_THREADS), 0, st, p, w2,
                       wo, P.K, P.TF, d, k_lo, count, fw.win, fw.stride);
    return;
  }
  const LongLossWs &w = wo;
  const auto tile = fw.win ? loss_long_beta_kernel<KIND, CKPT, true, false> : loss_long_beta_kernel<KIND, CKPT, false, false>;
  hipLaunchKernelGGL(tile, dim3((unsigned)((size_t)p.B * count)), dim3(LL_THREADS), 0, st, p, w2, w, P.K, P.TF, d, k_lo, count, fw.win, fw.stride);
}

template <int KIND>
hipError_t run_kind(const Problem &p, const LongLossPlan &P, double w2, const float *d_loss, float *loss, void *grad,
                    const LongLossWsOpt &wo, const LlWindow &fw, hipStream_t st) {
  const LongLossWs &w = wo;  // (the tiles take wo, everything else its base)
  if (p.T > 0) {
    for (int d = 0; d < P.launches; ++d) {
      int k_lo, count;
      long_loss_forward_diagonal(P, d, &k_lo, &count);
      if (grad) launch_alpha<KIND, 1>(p, P, w2, wo, fw, d, k_lo, count, st);
      else launch_alpha<KIND, 0>(p, P, w2, wo, fw, d, k_lo, count, st);
    }
  }
  if (fw.optional)
    hipLaunchKernelGGL((loss_long_finish_opt_kernel<KIND, false>), dim3((unsigned)((p.B + 255) / 256)), dim3(256), 0, st, p, w, P.K, P.TF, loss);
  else
    hipLaunchKernelGGL(loss_long_finish_kernel<KIND>, dim3((unsigned)((p.B + 255) / 256)), dim3(256), 0, st, p, w, P.K, loss);
  if (!grad || p.T == 0) return hipGetLastError();
  for (int e = 0; e < P.launches; ++e) {
    int d, k_lo, count;
    long_loss_backward_diagonal(P, e, &d, &k_lo, &count);
    launch_beta<KIND, false>(p, P, w2, wo, fw, d, k_lo, count, st);
  }
  const unsigned blocks = (unsigned)(((long)p.B * p.T + LLG_WAVES - 1) / LLG_WAVES);
  const auto rowk = fw.optional ? loss_long_row_kernel<KIND, true> : loss_long_row_kernel<KIND, false>;
  hipLaunchKernelGGL(rowk, dim3(blocks), dim3(64 * LLG_WAVES), 0, st, p, w, P.K, P.TF, d_loss, grad);
  return hipGetLastError();
}

// The checkpointed gradient (P.ckpt, grad != nullptr).  Forward: the alpha tiles keep no per-frame rows and
// leave their row out in the checkpoint of the tile.  Backward, per reverse anti-diagonal d: the alpha tiles of the diagonal run
// again from their checkpoints and save their rows into the ring, the beta tiles turn them into posteriors, and tile (0, d) having
// been the last of time block d, the row stage takes that block's frames.  The ring slot of time block d is next written on
// diagonal d - 1 (ctc_loss_long_plan.h), behind this row stage on the stream.
template <int KIND>
hipError_t run_kind_ckpt(const Problem &p, const LongLossPlan &P, double w2, const float *d_loss, float *loss, void *grad,
                         const LongLossWsOpt &wo, const LlWindow &fw, hipStream_t st, const LongPostOut *post = nullptr) {
  const LongLossWs &w = wo;  // (the tiles take wo, everything else its base)
  // post: ctc_amd_long_label_posterior, the posterior stage in the row stage's place (grad is nullptr)
  const bool per_label = post && p.U > 0 && (post->dur || post->peak);
  const unsigned stat_groups = per_label ? (unsigned)long_post_stat_groups(p.B, p.U) : 0u;
  auto post_stage = [&](int d, int nt) {
    const unsigned row_groups = (unsigned)long_post_row_groups(p.B, nt);
    if (row_groups + stat_groups == 0) return;
    const auto postk = fw.optional ? loss_long_post_kernel<KIND, true> : loss_long_post_kernel<KIND, false>;
    hipLaunchKernelGGL(postk, dim3(row_groups + stat_groups), dim3(64 * LONG_POST_WAVES), 0, st, p, w, *post, P.K, P.TF, d, nt, row_groups,
                       d == P.J - 1 ? 1 : 0, d == 0 ? 1 : 0);
  };
  if (p.T > 0) {
    for (int d = 0; d < P.launches; ++d) {
      int k_lo, count;
      long_loss_forward_diagonal(P, d, &k_lo, &count);
      launch_alpha<KIND, 2>(p, P, w2, wo, fw, d, k_lo, count, st);
    }
  }
  if (fw.optional)
    hipLaunchKernelGGL((loss_long_finish_opt_kernel<KIND, true>), dim3((unsigned)((p.B + 255) / 256)), dim3(256), 0, st, p, w, P.K, P.TF, loss);
  else
    hipLaunchKernelGGL(loss_long_finish_ckpt_kernel<KIND>, dim3((unsigned)((p.B + 255) / 256)), dim3(256), 0, st, p, w, P.K, P.TF, loss);
  if (p.T == 0) {
    if (post) post_stage(0, 0);  // (J == 1: the first and the last stage; nothing but the [B][U] outputs)
    return hipGetLastError();
  }
  for (int e = 0; e < P.launches; ++e) {
    int d, k_lo, count;
    long_loss_backward_diagonal(P, e, &d, &k_lo, &count);
    launch_alpha<KIND, 3>(p, P, w2, wo, fw, d, k_lo, count, st);
    launch_beta<KIND, true>(p, P, w2, wo, fw, d, k_lo, count, st);
    if (d < P.J) {
      const int t0 = d * P.TF, nt = p.T - t0 < P.TF ? p.T - t0 : P.TF;
      if (post) { post_stage(d, nt); continue; }
      const unsigned blocks = (unsigned)(((long)p.B * nt + LLG_WAVES - 1) / LLG_WAVES);
      const auto rowk = fw.optional ? loss_long_row_ckpt_kernel<KIND, true> : loss_long_row_ckpt_kernel<KIND, false>;
      hipLaunchKernelGGL(rowk, dim3(blocks), dim3(64 * LLG_WAVES), 0, st, p, w, P.K, P.TF, t0, nt, d_loss, grad);
    }
  }
  return hipGetLastError();
}

LongLossWsOpt long_loss_ws(char *ws, const LongLossPlan &P) {
  LongLossWsOpt w;
  w.col = reinterpret_cast<double *>(ws + P.off_col);
  w.row = reinterpret_cast<double *>(ws + P.off_row);
  w.stat = reinterpret_cast<float *>(ws + P.off_stat);
  w.logp = reinterpret_cast<double *>(ws + P.off_logp);
  w.flag = reinterpret_cast<int *>(ws + P.off_flag);
  w.colb = reinterpret_cast<double *>(ws + P.off_colb);
  w.rowb = reinterpret_cast<double *>(ws + P.off_rowb);
  w.rows = reinterpret_cast<double *>(ws + P.off_rows);
  w.col2 = reinterpret_cast<double *>(ws + P.off_col2);
  w.colb2 = reinterpret_cast<double *>(ws + P.off_colb2);
  return w;
}

}  // namespace

hipError_t run_loss_long(const Problem &p, const LongLossPlan &P, float wildcard_log_weight, const float *d_loss, float *loss, void *grad,
                         char *ws, hipStream_t st, const int32_t *frame_window, int window_stride, bool optional_wildcards) {
  if (p.kind < 0 || p.kind > 1 || (grad && !P.want_grad) || (P.ckpt && !grad)) return hipErrorInvalidValue;
  if (optional_wildcards && (frame_window || !P.opt)) return hipErrorInvalidValue;
  const LongLossWsOpt w = long_loss_ws(ws, P);
  const LlWindow fw{frame_window, window_stride, optional_wildcards};
  const double w2 = (double)wildcard_log_weight * LOG2E_D;
  if (P.ckpt)
    return p.kind == 0 ? run_kind_ckpt<0>(p, P, w2, d_loss, loss, grad, w, fw, st) : run_kind_ckpt<1>(p, P, w2, d_loss, loss, grad, w, fw, st);
  return p.kind == 0 ? run_kind<0>(p, P, w2, d_loss, loss, grad, w, fw, st) : run_kind<1>(p, P, w2, d_loss, loss, grad, w, fw, st);
}

hipError_t run_long_label_posterior(const Problem &p, const LongPostPlan &P, float wildcard_log_weight, float *loss, float *label_posterior,
                                    float *blank_posterior, float *duration, float *expected_frame, float *peak_posterior,
                                    int *peak_frame, char *ws, hipStream_t st, const int32_t *frame_window, int window_stride,
                                    bool optional_wildcards) {
  if (p.kind < 0 || p.kind > 1 || !P.L.ckpt || !duration != !expected_frame || !peak_posterior != !peak_frame) return hipErrorInvalidValue;
  if (optional_wildcards && (frame_window || !P.L.opt)) return hipErrorInvalidValue;
  const LongLossWsOpt w = long_loss_ws(ws, P.L);
  LongPostOut o;
  o.post = label_posterior; o.blk = blank_posterior;
  o.dur = duration; o.exf = expected_frame; o.peak = peak_posterior; o.peak_frame = peak_frame;
  o.acc = reinterpret_cast<double2 *>(ws + P.off_acc);
  o.pk = reinterpret_cast<float2 *>(ws + P.off_peak);
  const LlWindow fw{frame_window, window_stride, optional_wildcards};
  const double w2 = (double)wildcard_log_weight * LOG2E_D;
  return p.kind == 0 ? run_kind_ckpt<0>(p, P.L, w2, nullptr, loss, nullptr, w, fw, st, &o)
                     : run_kind_ckpt<1>(p, P.L, w2, nullptr, loss, nullptr, w, fw, st, &o);
}

}  // namespace ctc
