// Wildcard CTC loss and gradient from block checkpoints: ctc_amd_wildcard_loss_grad_ckpt (include/ctc_amd.h), DESIGN.md section 5.32.
// The gradient of ctc_wild_loss.hip (mandatory wildcard, no window, U <= 256) without a lattice row per frame in memory: two launches.
//
//   wild_ckpt_fwd_kernel  the MODE 1 alpha sweep of wild_loss_kernel (its file-local helpers and its body are repeated here; that file
//       stays as it is) with other stores: the chain's float64 state BEFORE frame k F for every block k of F frames aligned to frame 0,
//       the per-frame row statistics and log2 Z.  The arithmetic of the loss is the forward-only call's: the same bits.
//   wild_ckpt_bwd_kernel  one workgroup per utterance, six wavefronts, the K = ceil(T_b / F) blocks walked from the last (partial) one
//       down in K + 3 steps with ONE raw barrier each.  At step s
//         producers (waves 2..5)  gather the label emissions of block K - 1 - s into the emission ring (three buffers: a block is read
//                                 at step s + 1 by the recompute wave and at step s + 2 by the beta wave); the row statistics come
//                                 from the workspace, the row is not read.  Then the row stage of block K + 2 - s, whose posteriors
//                                 the beta wave finished in the previous step: wavefront pw takes frames pw, pw + 4, .. with bins of
//                                 its own, the arithmetic of wild_grad_row_kernel;
//         recompute (wave 1)      load checkpoint K - s, re-run the alpha step over that block's ring buffer, every frame's float64
//                                 row (MODE 1's layout) into one of two LDS row buffers;
//         beta (wave 0)           beta over block K + 1 - s, beta in registers, the alpha row of a frame from the LDS row buffer (read a
//                                 frame ahead), the posteriors of MODE 2 as float32 pairs into one of two LDS posterior blocks.
//       Nothing per frame reaches memory but the gradient row itself, which has one writer; no floating-point atomics.  The same
//       workgroup writes the zero rows of frames t >= T_b, of infeasible utterances and of a zero d_loss.
//
// LDS of the backward kernel, F * UP = 2048 (F = 32 / 16 / 8 frames at NL = 1 / 2 / 4), S = 2 classic / 1 simplified:
//   alpha rows   2 x F x (S UP + 2) doubles     66560 / 66048 / 65792 bytes classic, half of it + 2 F * 8 simplified
//   ring         3 x F x (UP + 4) floats        26112 / 25344 / 24960
//   posteriors   2 x F x (2 UP + 4) floats      33792 / 33280 / 33024
//   bins         4 x 1024 x 8 bytes             32768
//   labels       UP ints                          256 /   512 /  1024
// at most 159488 of the 163840 bytes a gfx950 workgroup may hold: one workgroup per CU.
//
// Label posteriors from the same checkpoints: ctc_amd_label_posterior_ckpt, DESIGN.md section 5.33.  Launch 1 is wild_ckpt_fwd_kernel.
//   wild_ckpt_post_kernel  the backward pipeline above (the same steps, barriers, gather, recompute and beta recursion) whose beta
//       wave leaves MODE 3's split in LDS -- per frame a plane of the labels' shares and a plane of the blank's, then the start
//       state's -- and whose producers' second job is a posterior writer: wavefront pw takes frames pw, pw + 4, .. of the block the
//       beta wave finished in the step before, lane l positions l, l + 64, ..: label_posterior[b, t, 0..U) as one contiguous run,
//       blank_posterior[b, t] summed over the wavefront in a fixed order, and the float32 values just written added to the lane's
//       float64 sums of duration and t * posterior.  The four writers' sums meet in LDS after the last step; the quotient is taken
//       in float64 and rounded once.  No statistics launch, no second read of the matrix, no atomics.
// LDS of the posterior kernel: alpha rows, ring and labels as above, and
//   posteriors   2 x F x (UP + UP + 4) floats   33792 / 33280 / 33024
//   partials     2 x 4 x UP doubles              4096 /  8192 / 16384
// 130816 / 133376 / 141184 bytes classic; the rest of the bins' 32 KB is left unused (deeper buffers would not shorten the beta chain).
//
// Star CTC from the same checkpoints: ctc_amd_star_loss_grad_ckpt, DESIGN.md section 5.34.  The two kernels carry OPT and XN as
// wild_loss_kernel does (the header of ctc_wild_loss.hip states the mathematics); this file is compiled twice more, with
// -DCTC_CKPT_OPT for (OPT, XN) = (true, false) and with -DCTC_STAR for (false, true) and (true, true).
//   OPT  two mask bits per position (`skip`, `skipo`) and the state two positions back in wk_alpha_step, from the lane's registers
//        or one more DPP shift; the beta wave is the mirror image; a last optional position makes the states before it end states.
//   XN   an utterance with an excluding star (`excl`) takes its row statistics as (max, sum of the rest) and keeps the sum of the
//        rest in the statistics' fourth float; both sweeps' producers write log2(1 - p_t(y)) into the ring slot of a wildcard
//        position and the chains add it to e_w.  The beta wave leaves c_i = Gamma_{t,i} 2^-slot in Gamma's place and the frame's
//        largest c in the posterior row's second spare float; the row stage splits its wavefront's bins into gamma's and D's, 512
//        columns a pass, and sums C through the row's last two spare floats as one 64-bit integer: the same LDS, byte for byte.
//
// Star label posteriors from the same checkpoints: ctc_amd_star_label_posterior_ckpt, DESIGN.md section 5.35.  wild_ckpt_post_kernel
// carries OPT and XN too, in the same two units: the gather, recompute and beta recursion of the star backward kernel with the
// output stage and the writer of the posterior kernel.  The shares are MODE 3's: a skipped star owns no frame, a frame entered over
// one belongs to the position entered; under XN the label plane holds Gamma itself (no c, no bins): the posterior kernel's LDS.
#include "ctc_wild_loss_ckpt.h"

#include "ctc_lane_ops.h"

namespace ctc {
namespace {

constexpr int WK_PW = 4;                          // producer wavefronts (both kernels)
constexpr int WK_FWD_THREADS = 64 * (1 + WK_PW);  // alpha sweep: + the chain
constexpr int WK_BWD_THREADS = 64 * (2 + WK_PW);  // backward sweep: + the beta wave and the recompute wave
constexpr int WK_RING = 4096;                     // alpha sweep: label emissions per ring buffer, as wild_loss_kernel
constexpr int WK_CH = 1024;                       // row stage: columns per pass
constexpr int WK_FIX = 40;                        // row stage: a posterior in units of 2^-40
constexpr double LOG2E_D = 1.44269504088896340736;

__device__ __forceinline__ float4 wk_row_load4(const char *row, int k, int dt) {
  if (dt == 0) return *reinterpret_cast<const float4 *>(row + (size_t)k * 4);
  const uint2 u = *reinterpret_cast<const uint2 *>(row + (size_t)k * 2);
  return make_float4(h16_to_f32((unsigned short)(u.x & 0xffffu), dt), h16_to_f32((unsigned short)(u.x >> 16), dt),
                     h16_to_f32((unsigned short)(u.y & 0xffffu), dt), h16_to_f32((unsigned short)(u.y >> 16), dt));
}
// the same four elements one by one (unaligned rows, V no multiple of 4): -inf past the row, which adds nothing to either statistic
__device__ __forceinline__ float4 wk_row_load4_elem(const char *row, int k, int V, int dt) {
  const float ninf = -__builtin_inff();
  return make_float4(row_load1(row, k, dt), k + 1 < V ? row_load1(row, k + 1, dt) : ninf, k + 2 < V ? row_load1(row, k + 2, dt) : ninf,
                     k + 3 < V ? row_load1(row, k + 3, dt) : ninf);
}
// running (max, sum of exp(x - max)) of one lane: four more elements (both access paths end here: identical bits)
__device__ __forceinline__ void wk_stat_add4(float &m, float &s, const float4 v) {
  const float mn = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
  s = s * fexp2((m - mn) * LOG2E) +
      ((fexp2((v.x - mn) * LOG2E) + fexp2((v.y - mn) * LOG2E)) + (fexp2((v.z - mn) * LOG2E) + fexp2((v.w - mn) * LOG2E)));
  m = mn;
}

// base-2 log(2^a + 2^b [+ 2^c]) of float64 operands that may be -inf (log 0): differences against the maximum, or against 0
// when every operand is -inf
__device__ __forceinline__ double wk_lse(double a, double b) {
  const double m = fmax(a, b);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2(fexp2((float)(a - mm)) + fexp2((float)(b - mm)));
}
__device__ __forceinline__ double wk_lse(double a, double b, double c) {
  const double m = fmax(fmax(a, b), c);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2((fexp2((float)(a - mm)) + fexp2((float)(b - mm))) + fexp2((float)(c - mm)));
}
// ... four and five operands (OPT): the further terms are added behind the first three, so -inf there leaves the bits as they are
__device__ __forceinline__ double wk_lse(double a, double b, double c, double d) {
  const double m = fmax(fmax(a, b), fmax(c, d));
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2(((fexp2((float)(a - mm)) + fexp2((float)(b - mm))) + fexp2((float)(c - mm))) + fexp2((float)(d - mm)));
}
__device__ __forceinline__ double wk_lse(double a, double b, double c, double d, double e) {
  const double m = fmax(fmax(fmax(a, b), fmax(c, d)), e);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2((((fexp2((float)(a - mm)) + fexp2((float)(b - mm))) + fexp2((float)(c - mm))) + fexp2((float)(d - mm))) +
                            fexp2((float)(e - mm)));
}

// XN: running (max, sum of exp(x - max) over the REST) of one lane, wl_rest_add4's update: the element that holds the maximum adds
// nothing, so 1 - p keeps its relative precision in a row with one dominant token.  m starts at the lowest finite float, s at 0
__device__ __forceinline__ void wk_rest_add1(float &m, float &s, const float v) {
  const float d = fexp2(-fabsf(v - m) * LOG2E);
  if (v > m) { s = (s + 1.f) * d; m = v; }
  else s += d;
}
__device__ __forceinline__ void wk_rest_add4(float &m, float &s, const float4 v) {
  wk_rest_add1(m, s, v.x); wk_rest_add1(m, s, v.y); wk_rest_add1(m, s, v.z); wk_rest_add1(m, s, v.w);
}
// XN: log2(1 - p_t(y)) of a token with logit v from the row's (max, sum of the rest, log2(sum of the rest + 1)): the sum of the rest
// where y holds the maximum, the whole sum less y's own term elsewhere; neither form cancels
__device__ __forceinline__ float wk_log2_rest(float v, float mx, float sr, float l2s) {
  const float num = v == mx ? sr : (sr + 1.f) - fexp2((v - mx) * LOG2E);
  return flog2(num) - l2s;
}

struct WkWs {
  double *ck;    // [B][ceil(T / F)][SRD] the chain's state before every block, in the layout of a MODE 1 row
  float *stat;   // [B][T][4] x[blank], row max, log2 sum exp(x - max) of every frame (XN, an excluding utterance: + the sum of the rest)
  double *logp;  // [B] log2 Z, -inf for an infeasible utterance
};
constexpr int wk_row_doubles(int kind, int UP) { return (kind == 0 ? 2 : 1) * UP + 2; }

// what a ring row says about its frame, in the lattice's units (base-2 logarithms of lp)
struct WkFrame {
  double Md, nl2s, eb, ew;
};
__device__ __forceinline__ WkFrame wk_frame_of(const float4 sv, bool lpin, double w2) {
  WkFrame fr;
  // logits: lp = x - max - ln sum; log-probabilities: lp = x
  fr.Md = lpin ? 0.0 : (double)sv.y;
  fr.nl2s = lpin ? 0.0 : -(double)sv.z;
  fr.eb = fma((double)sv.x - fr.Md, LOG2E_D, fr.nl2s);
  // e_w = w + ln sum_k exp(lp[t, k]): w for logits, w + LSE_t for log-probabilities; a row of -inf emits nothing
  fr.ew = sv.z == __builtin_inff() ? -__builtin_inf() : lpin ? w2 + fma((double)sv.y, LOG2E_D, (double)sv.z) : w2;
  return fr;
}

// the validated labels of utterance b: -1: no emission, WILD_LOSS_WILDCARD: a wildcard
// (OPT: WILD_LOSS_OPTIONAL: an optional wildcard; beside another one it is a bad label: no emission, no skip)
template <int UP, int THREADS, bool OPT = false>
__device__ __forceinline__ void wk_labels(const Problem &p, int b, int L, int tid, int *lab_s) {
  for (int i = tid; i < UP; i += THREADS) {
    int tok = -1;
    if (i < L) tok = label_at(p, label_row(p, b), i);
    int cls = tok == WILD_LOSS_WILDCARD ? WILD_LOSS_WILDCARD : emits(p, tok) ? tok : -1;
    if constexpr (OPT) {
      if (tok == WILD_LOSS_OPTIONAL) {
        const int32_t *const lr = label_row(p, b);
        const bool pair = (i > 0 && label_at(p, lr, i - 1) == WILD_LOSS_OPTIONAL) || (i + 1 < L && label_at(p, lr, i + 1) == WILD_LOSS_OPTIONAL);
        cls = pair ? -1 : WILD_LOSS_OPTIONAL;
      }
    }
    lab_s[i] = cls;
  }
}

// What a lane knows of its NL positions, set once from the validated labels.  wild: bit j = position lane * NL + j is a wildcard (of
// either kind); allow (classic): bit j = its label differs from the one before, or one of the two is a wildcard; OPT, bits 0..NL + 1
// (the beta wave looks two ahead): skip = the position before lane * NL + q is an optional wildcard, so q may be entered from two
// positions back, skipo = (classic) from the open state there too; last_opt = the last position is optional; XN: nx[j] = the token
// wildcard position j excludes (-1: none), excl = the utterance has such a position (the same in every thread)
template <int NL>
struct WkLane {
  int lab[NL], nx[NL];
  unsigned wild, allow, skip, skipo;
  bool last_opt, excl;
};
template <int KIND, int NL, bool OPT, bool XN>
__device__ __forceinline__ WkLane<NL> wk_lane_of(const int *lab_s, int lane, int L) {
  constexpr int UP = 64 * NL;
  auto is_wild = [](int tok) { return tok == WILD_LOSS_WILDCARD || (OPT && tok == WILD_LOSS_OPTIONAL); };
  WkLane<NL> m;
  m.wild = m.allow = m.skip = m.skipo = 0;
  m.last_opt = m.excl = false;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int i = lane * NL + j;
    m.lab[j] = lab_s[i];
    m.nx[j] = -1;
    if (is_wild(m.lab[j])) m.wild |= 1u << j;
    if (KIND == 0 && i > 0) {
      const int q = lab_s[i - 1];
      if (m.lab[j] != q || is_wild(m.lab[j]) || is_wild(q)) m.allow |= 1u << j;
    }
  }
  if constexpr (OPT) {
#pragma unroll
    for (int q = 0; q < NL + 2; ++q) {
      const int i = lane * NL + q;
      if (i >= 1 && i < UP && lab_s[i - 1] == WILD_LOSS_OPTIONAL) {
        m.skip |= 1u << q;
        if (KIND == 0 && i >= 2 && (lab_s[i] != lab_s[i - 2] || is_wild(lab_s[i]) || is_wild(lab_s[i - 2]))) m.skipo |= 1u << q;
      }
    }
    m.last_opt = L > 0 && lab_s[L - 1] == WILD_LOSS_OPTIONAL;
  }
  if constexpr (XN) {
    bool any = false;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int i = lane * NL + j;
      const int nt = i + 1 < UP ? lab_s[i + 1] : -1;  // (-1 past the label's length and for a label that does not emit)
      if (((m.wild >> j) & 1u) && nt >= 0) m.nx[j] = nt;
      any = any || m.nx[j] >= 0;
    }
    m.excl = __builtin_amdgcn_ballot_w64(any) != 0ull;
  }
  return m;
}

// one alpha step of a lane's NL positions over a frame with label emissions e: wild_loss_kernel's `consume`, without its stores
template <int KIND, int NL>
__device__ __forceinline__ void wk_alpha_step(double (&O)[NL], double (&C)[NL], double &cs, const float (&e)[NL], const WkFrame &fr,
                                              unsigned wild, unsigned allow) {
  const double NINF = -__builtin_inf();
  const double eb = fr.eb;
  auto em = [&](int j) { return ((wild >> j) & 1u) ? fr.ew : fma((double)e[j] - fr.Md, LOG2E_D, fr.nl2s); };
  if (KIND == 0) {
    const double pO = from_prev_lane(O[NL - 1], NINF);
    const double pC = from_prev_lane(C[NL - 1], cs);
#pragma unroll
    for (int j = NL - 1; j >= 0; --j) {
      const double qO = j > 0 ? O[j > 0 ? j - 1 : 0] : pO;
      const double qC = j > 0 ? C[j > 0 ? j - 1 : 0] : pC;
      const double a2 = ((allow >> j) & 1u) ? qO : NINF;
      const double o = wk_lse(O[j], qC, a2) + em(j);
      C[j] = wk_lse(C[j], O[j]) + eb;
      O[j] = o;
    }
  } else {
    const double pS = from_prev_lane(C[NL - 1], cs);
#pragma unroll
    for (int j = NL - 1; j >= 0; --j) {
      const double q = j > 0 ? C[j > 0 ? j - 1 : 0] : pS;
      C[j] = wk_lse(C[j] + (((wild >> j) & 1u) ? fr.ew : eb), q + em(j));
    }
  }
  cs += eb;
}

// ... with OPT and XN (the step above is kept as it is for the kernels without either): skip / skipo and the state two positions back;
// slot: XN in an utterance that excludes: the ring slot of a wildcard position is log2(1 - p_t(y)) and is added to e_w
template <int KIND, int NL, bool OPT, bool XN>
__device__ __forceinline__ void wk_star_step(double (&O)[NL], double (&C)[NL], double &cs, const float (&e)[NL], const WkFrame &fr,
                                              unsigned wild, unsigned allow, unsigned skip, unsigned skipo, bool slot) {
  const double NINF = -__builtin_inf();
  const double eb = fr.eb;
  auto ewj = [&](int j) { return XN && slot ? fr.ew + (double)e[j] : fr.ew; };
  auto em = [&](int j) { return ((wild >> j) & 1u) ? ewj(j) : fma((double)e[j] - fr.Md, LOG2E_D, fr.nl2s); };
  if (KIND == 0) {
    const double pO = from_prev_lane(O[NL - 1], NINF);
    const double pC = from_prev_lane(C[NL - 1], cs);
    // OPT: the position two before the lane's first: the previous lane's last but one (NL = 1: two lanes back; before lane 0 lies
    // the start state, and nothing before that)
    [[maybe_unused]] double pO2 = NINF, pC2 = NINF;
    if constexpr (OPT) {
      pO2 = from_prev_lane(NL == 1 ? pO : O[NL > 1 ? NL - 2 : 0], NINF);
      pC2 = from_prev_lane(NL == 1 ? pC : C[NL > 1 ? NL - 2 : 0], NINF);
    }
#pragma unroll
    for (int j = NL - 1; j >= 0; --j) {
      const double qO = j > 0 ? O[j > 0 ? j - 1 : 0] : pO;
      const double qC = j > 0 ? C[j > 0 ? j - 1 : 0] : pC;
      const double a2 = ((allow >> j) & 1u) ? qO : NINF;
      double o;
      if constexpr (OPT) {
        const double rO = j > 1 ? O[j > 1 ? j - 2 : 0] : j == 1 ? pO : pO2;
        const double rC = j > 1 ? C[j > 1 ? j - 2 : 0] : j == 1 ? pC : pC2;
        o = wk_lse(O[j], qC, a2, ((skip >> j) & 1u) ? rC : NINF, ((skipo >> j) & 1u) ? rO : NINF) + em(j);
      } else {
        o = wk_lse(O[j], qC, a2) + em(j);
      }
      C[j] = wk_lse(C[j], O[j]) + eb;
      O[j] = o;
    }
  } else {
    const double pS = from_prev_lane(C[NL - 1], cs);
    [[maybe_unused]] double pS2 = NINF;
    if constexpr (OPT) pS2 = from_prev_lane(NL == 1 ? pS : C[NL > 1 ? NL - 2 : 0], NINF);
#pragma unroll
    for (int j = NL - 1; j >= 0; --j) {
      const double q = j > 0 ? C[j > 0 ? j - 1 : 0] : pS;
      if constexpr (OPT) {
        const double r = j > 1 ? C[j > 1 ? j - 2 : 0] : j == 1 ? pS : pS2;
        C[j] = wk_lse(C[j] + (((wild >> j) & 1u) ? ewj(j) : eb), q + em(j), ((skip >> j) & 1u) ? r + em(j) : NINF);
      } else {
        C[j] = wk_lse(C[j] + (((wild >> j) & 1u) ? ewj(j) : eb), q + em(j));
      }
    }
  }
  cs += eb;
}

// ---- the alpha sweep with checkpoints ----
template <int KIND, int NL, bool OPT, bool XN>
__global__ __launch_bounds__(WK_FWD_THREADS) void wild_ckpt_fwd_kernel(const Problem p, const double w2, float *__restrict__ loss,
                                                                       const WkWs ws) {
  constexpr int UP = 64 * NL;
  constexpr int NS = (KIND == 0 ? 2 : 1) * NL;
  constexpr int SRD = wk_row_doubles(KIND, UP);
  constexpr int F = WK_RING / UP;            // frames per ring buffer: 64, 32, 16
  constexpr int FC = wild_ckpt_frames(NL);   // frames per checkpoint block: 32, 16, 8 (divides F)
  constexpr int RS = UP + 4;
  constexpr int FPW = F / WK_PW;
  constexpr int G = FPW < 4 ? FPW : 4;
  const double NINF = -__builtin_inf();

  __shared__ __attribute__((aligned(16))) float ring[2 * F * RS];
  __shared__ int lab_s[UP];

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int V = p.V, blank = p.blank, dt = p.xdtype;
  const bool lpin = p.wrt != 0;
  const int Tb = frame_count(p, b);
  int L = label_count(p, b);
  const bool too_long = too_many_labels(p, L);
  if (too_long) L = 0;

  wk_labels<UP, WK_FWD_THREADS, OPT>(p, b, L, tid, lab_s);
  __syncthreads();

  // (the kernels without OPT and XN set their masks in the statements they always had and keep their code)
  [[maybe_unused]] WkLane<NL> ln = {};
  int lab[NL];
  unsigned wild = 0, allow = 0;
  if constexpr (OPT || XN) {
    ln = wk_lane_of<KIND, NL, OPT, XN>(lab_s, lane, L);
    wild = ln.wild;
    allow = ln.allow;
  }
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    lab[j] = lab_s[lane * NL + j];
    if constexpr (!(OPT || XN)) {
      if (lab[j] == WILD_LOSS_WILDCARD) wild |= 1u << j;
    }
  }
  const bool excl = XN && ln.excl;
  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  const bool vec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (dt == 0 ? 15 : 7)) == 0;
  const int nck = (p.T + FC - 1) / FC;
  double *const myck = ws.ck + (size_t)b * nck * SRD;

  double O[NL], C[NL];
  double cs = 0.0;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    O[j] = NINF; C[j] = NINF;
    if constexpr (!(OPT || XN)) {
      const int i = lane * NL + j;
      if (KIND == 0 && i > 0) {
        const int a = lab_s[i], q = lab_s[i - 1];
        if (a != q || a == WILD_LOSS_WILDCARD || q == WILD_LOSS_WILDCARD) allow |= 1u << j;
      }
    }
  }

  auto produce = [&](int kb) {
    const int pw = wave - 1, q0 = kb * F;
    float *const rb = ring + (kb & 1) * F * RS;
    for (int f0 = pw * FPW; f0 < (pw + 1) * FPW; f0 += G) {
      if (q0 + f0 >= Tb) break;
      const char *row[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int q = q0 + f0 + g;  // past the utterance's end its last frame: valid memory whose results are never stored
        row[g] = xb + (size_t)((long)(q < Tb ? q : Tb - 1) * p.xst) * esz;
      }
      float e[G][NL], eb[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          const int tk = XN && lab[j] < 0 ? ln.nx[j] : lab[j];  // XN: a wildcard position gathers the token it excludes
          const float v = row_load1(row[g], tk >= 0 ? tk : blank, dt);
          e[g][j] = tk >= 0 ? v : -__builtin_inff();
        }
        eb[g] = row_load1(row[g], blank, dt);
      }
      float m[G], s[G];
#pragma unroll
      for (int g = 0; g < G; ++g) { m[g] = -3.402823466e38f; s[g] = 0.f; }
      for (int k = lane * 4; k < V; k += 256) {
        float4 v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) v[g] = vec ? wk_row_load4(row[g], k, dt) : wk_row_load4_elem(row[g], k, V, dt);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (excl) wk_rest_add4(m[g], s[g], v[g]);
          else wk_stat_add4(m[g], s[g], v[g]);
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float M = wave_max(m[g]);
        float l2s;
        [[maybe_unused]] float Sr = 0.f, Mr = 0.f;  // XN: the sum of the rest, the row's own maximum
        if (excl) {
          // the lowest lane at the maximum keeps its 1 out; every other lane's own maximum is part of the rest
          const unsigned long long at = __builtin_amdgcn_ballot_w64(m[g] == M);
          const bool own = lane == (int)__builtin_ctzll(at);
          Sr = wave_sum(own ? s[g] : (s[g] + 1.f) * fexp2((m[g] - M) * LOG2E));
          Mr = M;
          l2s = flog2(Sr + 1.f);
          if (!(M > -3.402823466e38f)) { M = 0.f; l2s = __builtin_inff(); }  // a row of -inf
        } else {
          const float S = wave_sum(s[g] * fexp2((m[g] - M) * LOG2E));
          l2s = flog2(S);
          if (!(S > 0.f)) { M = 0.f; l2s = __builtin_inff(); }  // a row of -inf: every emission of the frame is -inf
        }
        if (q0 + f0 + g < Tb) {
          float *const r = rb + (f0 + g) * RS;
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            float v = e[g][j];
            if constexpr (XN) {  // log2(1 - p_t(y)) for a wildcard position that excludes y, 0 for one that excludes nothing
              if (excl && ((wild >> j) & 1u)) v = ln.nx[j] >= 0 ? wk_log2_rest(v, Mr, Sr, l2s) : 0.f;
            }
            r[lane * NL + j] = v;
          }
          if (lane == 0) {
            *reinterpret_cast<float4 *>(r + UP) = make_float4(eb[g], M, l2s, 0.f);
            *reinterpret_cast<float4 *>(ws.stat + ((size_t)b * p.T + q0 + f0 + g) * 4) = make_float4(eb[g], M, l2s, Sr);
          }
        }
      }
    }
  };

  auto consume = [&](int kb) {
    const int t0 = kb * F;
    const int nf = Tb - t0 < F ? Tb - t0 : F;
    const float *const rb = ring + (kb & 1) * F * RS;
    for (int f = 0; f < nf; ++f) {
      if ((f & (FC - 1)) == 0) {  // the state BEFORE the first frame of a checkpoint block
        double *const r = myck + (size_t)((t0 + f) / FC) * SRD;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          if (KIND == 0) *reinterpret_cast<double2 *>(r + lane * NS + 2 * j) = make_double2(O[j], C[j]);
          else r[lane * NS + j] = C[j];
        }
        if (lane == 0) r[SRD - 2] = cs;
      }
      const float *const rr = rb + f * RS;
      float e[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) e[j] = rr[lane * NL + j];
      const WkFrame fr = wk_frame_of(*reinterpret_cast<const float4 *>(rr + UP), lpin, w2);
      if constexpr (OPT || XN) wk_star_step<KIND, NL, OPT, XN>(O, C, cs, e, fr, wild, allow, ln.skip, ln.skipo, excl);
      else wk_alpha_step<KIND, NL>(O, C, cs, e, fr, wild, allow);
    }
  };

  const int nb = (Tb + F - 1) / F;
  if (wave > 0 && nb > 0) produce(0);
  __syncthreads();
  for (int kb = 0; kb < nb; ++kb) {
    if (wave == 0) consume(kb);
    else if (kb + 1 < nb) produce(kb + 1);
    __syncthreads();
  }

  if (wave == 0) {
    const int i = L - 1, jj = i & (NL - 1);
    double cv = C[0], ov = O[0];
#pragma unroll
    for (int j = 1; j < NL; ++j)
      if (j == jj) { cv = C[j]; ov = O[j]; }
    double v = cs;
    if (L > 0) v = KIND == 0 ? wk_lse(ov, cv) : cv;
    if constexpr (OPT) {  // the last position may be empty: the states before it end the utterance too (every lane takes part)
      if (ln.last_opt) {
        const int i2 = L >= 2 ? L - 2 : 0, j2 = i2 & (NL - 1);
        double c2 = C[0], o2 = O[0];
#pragma unroll
        for (int j = 1; j < NL; ++j)
          if (j == j2) { c2 = C[j]; o2 = O[j]; }
        c2 = __shfl(c2, i2 / NL);
        o2 = __shfl(o2, i2 / NL);
        const double v2 = L == 1 ? cs : KIND == 0 ? wk_lse(o2, c2) : c2;
        v = wk_lse(v, v2);
      }
    }
    if (too_long) v = NINF;
    if (lane == (L > 0 ? i / NL : 0)) {
      loss[b] = (float)(0.0 - v * LN2_D);  // (-inf: +inf; an empty utterance: +0)
      ws.logp[b] = v;
    }
  }
}

// four consecutive elements of a gradient row from column k, in its element type; element-wise where the row is not aligned
__device__ __forceinline__ void wk_grad_put4(char *g, int k, int V, int gdt, bool gvec, const float4 r) {
  if (gdt == 0) {
    if (gvec) { *reinterpret_cast<float4 *>(g + (size_t)k * 4) = r; return; }
    float *const o = reinterpret_cast<float *>(g);
    o[k] = r.x;
    if (k + 1 < V) o[k + 1] = r.y;
    if (k + 2 < V) o[k + 2] = r.z;
    if (k + 3 < V) o[k + 3] = r.w;
    return;
  }
  auto cv = [&](float f) { return gdt == 1 ? f32_to_bf16(f) : f32_to_f16(f); };
  const unsigned short h0 = cv(r.x), h1 = cv(r.y), h2 = cv(r.z), h3 = cv(r.w);
  if (gvec) {
    *reinterpret_cast<uint2 *>(g + (size_t)k * 2) = make_uint2((unsigned)h0 | ((unsigned)h1 << 16), (unsigned)h2 | ((unsigned)h3 << 16));
    return;
  }
  unsigned short *const o = reinterpret_cast<unsigned short *>(g);
  o[k] = h0;
  if (k + 1 < V) o[k + 1] = h1;
  if (k + 2 < V) o[k + 2] = h2;
  if (k + 3 < V) o[k + 3] = h3;
}

// ---- the pipelined backward sweep ----
template <int KIND, int NL, bool OPT, bool XN>
__global__ __launch_bounds__(WK_BWD_THREADS) void wild_ckpt_bwd_kernel(const Problem p, const double w2, const float *__restrict__ d_loss,
                                                                       const WkWs ws, void *__restrict__ grad) {
  constexpr int UP = 64 * NL;
  constexpr int NS = (KIND == 0 ? 2 : 1) * NL;
  constexpr int SRD = wk_row_doubles(KIND, UP);
  constexpr int F = wild_ckpt_frames(NL);
  constexpr int RS = UP + 4;      // ring row: UP label emissions, then the frame's statistics
  // posterior row: a float32 pair per position, then the start state's blank posterior; XN: then the frame's largest c, and the
  // last two floats are the row stage's 64-bit sum of c
  constexpr int PR = 2 * UP + 4;
  constexpr int FPW = F / WK_PW;  // frames per producer wavefront and block: 8, 4, 2
  constexpr int G = FPW < 4 ? FPW : 4;
  static_assert(F >= 4 && F % WK_PW == 0, "every producer wavefront takes whole frames of a block");
  const double NINF = -__builtin_inf();

  __shared__ __attribute__((aligned(16))) double arow[2 * F * SRD];
  __shared__ __attribute__((aligned(16))) float ring[3 * F * RS];
  __shared__ __attribute__((aligned(16))) float pst[2 * F * PR];
  __shared__ unsigned long long bins_all[WK_PW][WK_CH];
  __shared__ int lab_s[UP];

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int V = p.V, blank = p.blank, dt = p.xdtype, gdt = p.gdtype;
  const bool lpin = p.wrt != 0;
  const int Tb = frame_count(p, b);
  const int esz = dt == 0 ? 4 : 2, gesz = gdt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  char *const gb = reinterpret_cast<char *>(grad) + (size_t)((long)b * p.gsb) * gesz;
  const bool xvec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (dt == 0 ? 15 : 7)) == 0;
  const bool gvec = ((V | p.gsb | p.gst) & 3) == 0 && (reinterpret_cast<uintptr_t>(grad) & (gdt == 0 ? 15 : 7)) == 0;

  // an infinite loss contributes nothing and its d_loss is not interpreted; a weight of zero: +0 throughout
  const double lP = ws.logp[b];
  const bool feasible = lP > NINF && lP < -NINF;
  const float dl = d_loss ? d_loss[b] : 1.f;
  // padded frames, every frame of an infeasible utterance or of a zero weight: exactly zero
  const int Tz = (feasible && dl != 0.f) ? Tb : 0;
  for (int t = Tz + wave; t < p.T; t += WK_BWD_THREADS / 64) {
    char *const g = gb + (size_t)((long)t * p.gst) * gesz;
    for (int k = lane * 4; k < V; k += 256) wk_grad_put4(g, k, V, gdt, gvec, make_float4(0.f, 0.f, 0.f, 0.f));
  }
  if (Tz == 0) return;  // (the same verdict in every wavefront: nobody waits at a barrier)

  const int L = label_count(p, b);  // (feasible: L <= U <= UP)
  wk_labels<UP, WK_BWD_THREADS, OPT>(p, b, L, tid, lab_s);
  __syncthreads();

  [[maybe_unused]] WkLane<NL> ln = {};
  int lab[NL];
  unsigned wild = 0, allow = 0;
  if constexpr (OPT || XN) {
    ln = wk_lane_of<KIND, NL, OPT, XN>(lab_s, lane, L);
    wild = ln.wild;
    allow = ln.allow;
  }
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int i = lane * NL + j;
    lab[j] = lab_s[i];
    if constexpr (!(OPT || XN)) {
      if (lab[j] == WILD_LOSS_WILDCARD) wild |= 1u << j;
      if (KIND == 0 && i > 0) {
        const int q = lab_s[i - 1];
        if (lab[j] != q || lab[j] == WILD_LOSS_WILDCARD || q == WILD_LOSS_WILDCARD) allow |= 1u << j;
      }
    }
  }
  const int allow_nx = KIND == 0 ? fused::from_next_lane_i((int)(allow & 1u), 0) : 0;
  [[maybe_unused]] const unsigned skip = ln.skip, skipo = ln.skipo;
  const bool excl = XN && ln.excl;

  const int K = (Tb + F - 1) / F;       // blocks of the utterance
  const int nck = (p.T + F - 1) / F;    // checkpoint rows per utterance
  auto frames_of = [&](int kb) { return Tb - kb * F < F ? Tb - kb * F : F; };

  // ---- producers, first job: the emissions of block kb into its ring buffer, its statistics from the workspace ----
  auto gather = [&](int kb) {
    const int pw = wave - 2, t0 = kb * F;
    float *const rb = ring + (kb % 3) * F * RS;
    for (int f0 = pw * FPW; f0 < (pw + 1) * FPW; f0 += G) {
      if (t0 + f0 >= Tb) break;
      float e[G][NL];
      float4 sv[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int q = t0 + f0 + g, t = q < Tb ? q : Tb - 1;  // past the utterance's end its last frame: never stored
        const char *const row = xb + (size_t)((long)t * p.xst) * esz;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          const int tk = XN && lab[j] < 0 ? ln.nx[j] : lab[j];  // XN: a wildcard position gathers the token it excludes
          const float v = row_load1(row, tk >= 0 ? tk : blank, dt);
          e[g][j] = tk >= 0 ? v : -__builtin_inff();
        }
        sv[g] = *reinterpret_cast<const float4 *>(ws.stat + ((size_t)b * p.T + t) * 4);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (t0 + f0 + g < Tb) {
          float *const r = rb + (f0 + g) * RS;
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            float v = e[g][j];
            if constexpr (XN) {  // the alpha sweep's slot from its statistics: (max, log2(rest + 1), rest) in .y, .z, .w
              if (excl && ((wild >> j) & 1u)) v = ln.nx[j] >= 0 ? wk_log2_rest(v, sv[g].y, sv[g].w, sv[g].z) : 0.f;
            }
            r[lane * NL + j] = v;
          }
          if (lane == 0) *reinterpret_cast<float4 *>(r + UP) = sv[g];
        }
      }
    }
  };

  // ---- producers, second job: the row stage of block kb from its posterior block; wild_grad_row_kernel's arithmetic ----
  auto rows = [&](int kb) {
    const int pw = wave - 2, nf = frames_of(kb);
    unsigned long long *const bins = bins_all[pw];
    for (int f = pw; f < nf; f += WK_PW) {
      const int t = kb * F + f;
      const float *const pr = pst + ((kb & 1) * F + f) * PR;
      const char *const x = xb + (size_t)((long)t * p.xst) * esz;
      char *const g = gb + (size_t)((long)t * p.gst) * gesz;
      const float4 sv = *reinterpret_cast<const float4 *>(ws.stat + ((size_t)b * p.T + t) * 4);
      const float mx = sv.y, l2s = sv.z;
      if constexpr (XN) {
        // An utterance that excludes: the beta wave left c_i = Gamma_{t,i} / (1 - p_t(y_i)) in Gamma's place and the frame's largest c
        // behind the start state's posterior.  gamma's bins in the first half of the wavefront's bins, D's (c scattered by y_i) in the
        // second: passes of 512 columns.  c is not bounded by 1: the unit of its bins comes from the frame.  cmax < 2^ex, so
        // c 2^sh < 2^50 and 256 of them < 2^58.  C, the sum of c in that unit, meets in the row's last two floats: integer, no order
        if (excl) {
          constexpr int CH = WK_CH / 2;
          unsigned long long *const dbins = bins + CH;
          unsigned long long *const csum = reinterpret_cast<unsigned long long *>(pst + ((kb & 1) * F + f) * PR + 2 * UP + 2);
          int ex;
          (void)__builtin_frexpf(pr[2 * UP + 1], &ex);
          const int sh = 50 - ex;
          float blk = 0.f;
          unsigned long long ctot = 0ull;
          for (int c0 = 0; c0 < V; c0 += CH) {
#pragma unroll
            for (int q = 0; q < WK_CH / 64; ++q) bins[lane + 64 * q] = 0ull;  // (both halves)
            if (c0 == 0 && lane == 0) *csum = 0ull;
            wave_lds_fence();
            unsigned long long cl = 0ull;
            for (int i = lane; i < L; i += 64) {
              const float2 pq = *reinterpret_cast<const float2 *>(pr + 2 * i);
              const int tok = lab_s[i];  // (-1: no emission)
              const bool w = tok == WILD_LOSS_WILDCARD || (OPT && tok == WILD_LOSS_OPTIONAL);
              const unsigned rel = (unsigned)(tok - c0);
              if (tok >= 0 && rel < (unsigned)CH)
                atomicAdd(&bins[rel], (unsigned long long)__float2ll_rn(__builtin_ldexpf(pq.x, WK_FIX)));
              if (w) {
                const int y = i + 1 < UP ? lab_s[i + 1] : -1;  // the token position i excludes (negative: none)
                const unsigned long long q = (unsigned long long)__float2ll_rn(__builtin_ldexpf(KIND == 1 ? pq.x + pq.y : pq.x, sh));
                cl += q;
                if (y >= 0 && (unsigned)(y - c0) < (unsigned)CH) atomicAdd(&dbins[y - c0], q);
              }
              if (c0 == 0 && !(KIND == 1 && w)) blk += pq.y;
            }
            if (c0 == 0) {
              if (lane == 0) blk += pr[2 * UP];
              blk = wave_sum(blk);
              atomicAdd(csum, cl);
            }
            wave_lds_fence();
            if (c0 == 0) ctot = *csum;
#pragma unroll
            for (int q = 0; q < CH / 256; ++q) {
              const int k = c0 + lane * 4 + 256 * q;
              if (k < V) {
                const float4 xv = xvec ? wk_row_load4(x, k, dt) : wk_row_load4_elem(x, k, V, dt);
                float o[4];
                const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                  const float bin = __builtin_ldexpf(__ll2float_rn((long long)bins[k - c0 + cc]), -WK_FIX) + (k + cc == blank ? blk : 0.f);
                  // C - D(k): an integer difference, exact
                  const float cd = __builtin_ldexpf(__ll2float_rn((long long)(ctot - dbins[k - c0 + cc])), -sh);
                  const float c = !lpin ? 1.f - cd : -cd;
                  const float sm = c == 0.f ? 0.f : c * fexp2((xs[cc] - mx) * LOG2E - l2s);
                  o[cc] = dl * (sm - bin);
                }
                wk_grad_put4(g, k, V, gdt, gvec, make_float4(o[0], o[1], o[2], o[3]));
              }
            }
            wave_lds_fence();
          }
          continue;
        }
      }
      float blk = 0.f, gam = 0.f;  // the blank's share and Gamma_t, lane-wise partial sums in a fixed order
      for (int c0 = 0; c0 < V; c0 += WK_CH) {
#pragma unroll
        for (int q = 0; q < WK_CH / 64; ++q) bins[lane + 64 * q] = 0ull;
        wave_lds_fence();
        for (int i = lane; i < L; i += 64) {
          const float2 pq = *reinterpret_cast<const float2 *>(pr + 2 * i);
          const int tok = lab_s[i];  // (-1: no emission)
          const bool w = tok == WILD_LOSS_WILDCARD || (OPT && tok == WILD_LOSS_OPTIONAL);
          const unsigned rel = (unsigned)(tok - c0);
          if (tok >= 0 && rel < (unsigned)WK_CH)
            atomicAdd(&bins[rel], (unsigned long long)__float2ll_rn(__builtin_ldexpf(pq.x, WK_FIX)));
          if (c0 == 0) {
            if (w) gam += pq.x;
            if (KIND == 1 && w) gam += pq.y;
            else blk += pq.y;
          }
        }
        if (c0 == 0) {
          if (lane == 0) blk += pr[2 * UP];
          blk = wave_sum(blk);
          gam = wave_sum(gam);
        }
        wave_lds_fence();
        // logits: (1 - Gamma) softmax - gamma;  log-probabilities: -Gamma exp(x - LSE) - gamma
        const float c = !lpin ? 1.f - gam : -gam;
#pragma unroll
        for (int q = 0; q < WK_CH / 256; ++q) {
          const int k = c0 + lane * 4 + 256 * q;
          if (k < V) {
            const float4 xv = xvec ? wk_row_load4(x, k, dt) : wk_row_load4_elem(x, k, V, dt);
            float o[4];
            const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
              const float bin = __builtin_ldexpf(__ll2float_rn((long long)bins[k - c0 + cc]), -WK_FIX) + (k + cc == blank ? blk : 0.f);
              const float sm = c == 0.f ? 0.f : c * fexp2((xs[cc] - mx) * LOG2E - l2s);
              o[cc] = dl * (sm - bin);
            }
            wk_grad_put4(g, k, V, gdt, gvec, make_float4(o[0], o[1], o[2], o[3]));
          }
        }
        wave_lds_fence();
      }
    }
  };

  // ---- recompute wave: alpha over block kb from its checkpoint, every frame's row into the block's LDS row buffer ----
  auto recompute = [&](int kb) {
    const double *const r = ws.ck + ((size_t)b * nck + kb) * SRD;
    double O[NL], C[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      if (KIND == 0) {
        const double2 v = *reinterpret_cast<const double2 *>(r + lane * NS + 2 * j);
        O[j] = v.x; C[j] = v.y;
      } else {
        O[j] = NINF; C[j] = r[lane * NS + j];
      }
    }
    double cs = r[SRD - 2];
    const int nf = frames_of(kb);
    const float *const rb = ring + (kb % 3) * F * RS;
    double *const ab = arow + (size_t)(kb & 1) * F * SRD;
    for (int f = 0; f < nf; ++f) {
      const float *const rr = rb + f * RS;
      double *const a = ab + f * SRD;
      float e[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) e[j] = rr[lane * NL + j];
      const WkFrame fr = wk_frame_of(*reinterpret_cast<const float4 *>(rr + UP), lpin, w2);
      if (KIND == 1) {  // the state BEFORE the frame
#pragma unroll
        for (int j = 0; j < NL; ++j) a[lane * NS + j] = C[j];
        if (lane == 0) a[SRD - 2] = cs;
      }
      if constexpr (OPT || XN) wk_star_step<KIND, NL, OPT, XN>(O, C, cs, e, fr, wild, allow, ln.skip, ln.skipo, excl);
      else wk_alpha_step<KIND, NL>(O, C, cs, e, fr, wild, allow);
      if (KIND == 0) {  // the state AFTER the frame
#pragma unroll
        for (int j = 0; j < NL; ++j) *reinterpret_cast<double2 *>(a + lane * NS + 2 * j) = make_double2(O[j], C[j]);
        if (lane == 0) a[SRD - 2] = cs;
      }
    }
  };

  // ---- beta wave: the posteriors of block kb's frames, last first, and beta back over each; wild_loss_kernel's MODE 2 ----
  double bO[NL], bC[NL];  // beta: the mass of the frames still to come; behind the last frame only the end states have any
#pragma unroll
  for (int j = 0; j < NL; ++j) bO[j] = bC[j] = (lane * NL + j == L - 1 || (OPT && ln.last_opt && lane * NL + j == L - 2)) ? 0.0 : NINF;
  double bcs = (L == 0 || (OPT && ln.last_opt && L == 1)) ? 0.0 : NINF;
  auto post = [&](double l2) { return fexp2((float)(l2 - lP)); };
  auto beta_block = [&](int kb) {
    const int nf = frames_of(kb);
    const float *const rb = ring + (kb % 3) * F * RS;
    const double *const ab = arow + (size_t)(kb & 1) * F * SRD;
    float *const pb = pst + (size_t)(kb & 1) * F * PR;
    double An[NS], Acsn;
    auto load_row = [&](int f) {
      const double *const a = ab + f * SRD;
#pragma unroll
      for (int q = 0; q < NS; ++q) An[q] = a[lane * NS + q];
      Acsn = a[SRD - 2];
    };
    load_row(nf - 1);
    for (int f = nf - 1; f >= 0; --f) {
      const float *const rr = rb + f * RS;
      float *const o = pb + f * PR;
      float e[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) e[j] = rr[lane * NL + j];
      const WkFrame fr = wk_frame_of(*reinterpret_cast<const float4 *>(rr + UP), lpin, w2);
      const double eb = fr.eb;
      // (XN, in an utterance that excludes: the ring slot of a wildcard position is log2(1 - p_t(y)))
      auto ewj = [&](int j) { return excl ? fr.ew + (double)e[j] : fr.ew; };
      auto em = [&](int j) { return ((wild >> j) & 1u) ? ewj(j) : fma((double)e[j] - fr.Md, LOG2E_D, fr.nl2s); };
      double A[NS];
#pragma unroll
      for (int q = 0; q < NS; ++q) A[q] = An[q];
      const double Acs = Acsn;
      if (f > 0) load_row(f - 1);  // the next frame's row, a frame ahead
      [[maybe_unused]] float cm = 0.f;  // XN: the frame's largest c
      if (KIND == 0) {
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          float g = post(A[2 * j] + bO[j]);
          if constexpr (XN) {  // a wildcard's Gamma becomes c = Gamma / (1 - p): the slot is log2(1 - p)
            if (excl && ((wild >> j) & 1u)) {
              g = g > 0.f ? g * fexp2(-e[j]) : 0.f;
              cm = fmaxf(cm, g);
            }
          }
          *reinterpret_cast<float2 *>(o + 2 * (lane * NL + j)) = make_float2(g, post(A[2 * j + 1] + bC[j]));
        }
        if (lane == 0) o[2 * UP] = post(Acs + bcs);
        // beta back over the frame: x = what entering O[i] with this frame is worth
        double x = bO[0] + em(0);
        const double xl = from_next_lane(x, NINF);
        if constexpr (OPT) {
          // the mirror image of the alpha step: what entering the open states one and two positions ahead is worth; beyond the
          // lane's own they are the next lane's first two (NL = 1: the next two lanes')
          double x1 = NL > 1 ? bO[NL > 1 ? 1 : 0] + em(NL > 1 ? 1 : 0) : xl;
          const double xl2 = from_next_lane(x1, NINF);
          bcs = wk_lse(bcs + eb, x, ((skip >> 1) & 1u) ? x1 : NINF);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double x2 = j + 2 < NL ? bO[j + 2 < NL ? j + 2 : 0] + em(j + 2 < NL ? j + 2 : 0) : j + 2 == NL ? xl : xl2;
            const bool al = j + 1 < NL ? ((allow >> (j + 1)) & 1u) != 0 : allow_nx != 0;
            const double cb = bC[j] + eb;
            bO[j] = wk_lse(x, cb, al ? x1 : NINF, ((skipo >> (j + 2)) & 1u) ? x2 : NINF);
            bC[j] = wk_lse(cb, x1, ((skip >> (j + 2)) & 1u) ? x2 : NINF);
            x = x1;
            x1 = x2;
          }
        } else {
          bcs = wk_lse(bcs + eb, x);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double xn = j + 1 < NL ? bO[j + 1 < NL ? j + 1 : 0] + em(j + 1 < NL ? j + 1 : 0) : xl;
            const bool al = j + 1 < NL ? ((allow >> (j + 1)) & 1u) != 0 : allow_nx != 0;
            const double cb = bC[j] + eb;
            bO[j] = wk_lse(x, cb, al ? xn : NINF);
            bC[j] = wk_lse(cb, xn);
            x = xn;
          }
        }
      } else {
        const double ap0 = from_prev_lane(A[NL - 1], Acs);
        [[maybe_unused]] double ap00 = NINF;  // OPT: alpha two positions before the lane's first
        if constexpr (OPT) ap00 = from_prev_lane(NL == 1 ? ap0 : A[NL > 1 ? NL - 2 : 0], NINF);
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          double ap = j > 0 ? A[j > 0 ? j - 1 : 0] : ap0;
          if constexpr (OPT) {  // entered from one position back or, over an optional wildcard, from two
            const double ap2 = j > 1 ? A[j > 1 ? j - 2 : 0] : j == 1 ? ap0 : ap00;
            ap = wk_lse(ap, ((skip >> j) & 1u) ? ap2 : NINF);
          }
          const bool wj = ((wild >> j) & 1u) != 0;
          const double h = wj ? ewj(j) : eb;
          float pe = post(ap + em(j) + bC[j]), ps = post(A[j] + h + bC[j]);
          if constexpr (XN) {  // a wildcard's two shares of Gamma become those of c = Gamma / (1 - p)
            if (excl && wj) {
              const float sc = fexp2(-e[j]);
              pe = pe > 0.f ? pe * sc : 0.f;
              ps = ps > 0.f ? ps * sc : 0.f;
              cm = fmaxf(cm, pe + ps);
            }
          }
          *reinterpret_cast<float2 *>(o + 2 * (lane * NL + j)) = make_float2(pe, ps);
        }
        if (lane == 0) o[2 * UP] = post(Acs + eb + bcs);
        double x = bC[0] + em(0);
        const double xl = from_next_lane(x, NINF);
        if constexpr (OPT) {
          double x1 = NL > 1 ? bC[NL > 1 ? 1 : 0] + em(NL > 1 ? 1 : 0) : xl;
          const double xl2 = from_next_lane(x1, NINF);
          bcs = wk_lse(bcs + eb, x, ((skip >> 1) & 1u) ? x1 : NINF);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double x2 = j + 2 < NL ? bC[j + 2 < NL ? j + 2 : 0] + em(j + 2 < NL ? j + 2 : 0) : j + 2 == NL ? xl : xl2;
            bC[j] = wk_lse(bC[j] + (((wild >> j) & 1u) ? ewj(j) : eb), x1, ((skip >> (j + 2)) & 1u) ? x2 : NINF);
            x1 = x2;
          }
        } else {
          bcs = wk_lse(bcs + eb, x);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double xn = j + 1 < NL ? bC[j + 1 < NL ? j + 1 : 0] + em(j + 1 < NL ? j + 1 : 0) : xl;
            bC[j] = wk_lse(bC[j] + (((wild >> j) & 1u) ? ewj(j) : eb), xn);
            x = xn;
          }
        }
      }
      if constexpr (XN) {
        if (excl) {
          cm = wave_max(cm);
          if (lane == 0) o[2 * UP + 1] = cm;
        }
      }
    }
  };

  // every wavefront derives the same K: the barrier counts match by construction
  for (int s = 0; s <= K + 2; ++s) {
    if (wave == 0) {
      const int kb = K + 1 - s;
      if (kb >= 0 && kb < K) beta_block(kb);
    } else if (wave == 1) {
      const int kb = K - s;
      if (kb >= 0 && kb < K) recompute(kb);
    } else {
      const int kg = K - 1 - s, kr = K + 2 - s;
      if (kg >= 0) gather(kg);
      if (kr >= 0 && kr < K) rows(kr);
    }
    fused::block_barrier();
  }
}

// ---- label posteriors from the same checkpoints: the backward pipeline with a posterior writer as its last stage ----
struct WkPost {
  float *post;  // [B][T][U] label_posterior
  float *blk;   // [B][T] blank_posterior
  float *dur;   // [B][U] duration, or nullptr: no statistics
  float *exf;   // [B][U] expected_frame (given together with dur)
};

// a lane's NL consecutive floats of an LDS plane in one store
template <int NL>
__device__ __forceinline__ void wk_put_run(float *o, const float (&v)[NL]) {
  if constexpr (NL == 4) *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
  else if constexpr (NL == 2) *reinterpret_cast<float2 *>(o) = make_float2(v[0], v[1]);
  else o[0] = v[0];
}

// The gather, recompute and beta roles are wild_ckpt_bwd_kernel's, statement for statement (that kernel keeps its code, so they are
// repeated and not shared); what differs is what the beta wave leaves in LDS and who takes it from there.  OPT and XN as in that
// kernel (section 5.35); under XN the label plane holds Gamma itself, and the four spare floats of a posterior row keep their use.
template <int KIND, int NL, bool OPT, bool XN>
__global__ __launch_bounds__(WK_BWD_THREADS) void wild_ckpt_post_kernel(const Problem p, const double w2, const WkWs ws, const WkPost out) {
  constexpr int UP = 64 * NL;
  constexpr int NS = (KIND == 0 ? 2 : 1) * NL;
  constexpr int SRD = wk_row_doubles(KIND, UP);
  constexpr int F = wild_ckpt_frames(NL);
  constexpr int RS = UP + 4;      // ring row: UP label emissions, then the frame's statistics
  constexpr int PR = 2 * UP + 4;  // posterior row: the plane of the labels' shares, the plane of the blank's, the start state's
  constexpr int FPW = F / WK_PW;  // frames per producer wavefront and block: 8, 4, 2
  constexpr int G = FPW < 4 ? FPW : 4;
  static_assert(F >= 4 && F % WK_PW == 0, "every producer wavefront takes whole frames of a block");
  static_assert(UP <= WK_BWD_THREADS, "one thread per label position combines the statistics");
  const double NINF = -__builtin_inf();

  __shared__ __attribute__((aligned(16))) double arow[2 * F * SRD];
  __shared__ __attribute__((aligned(16))) float ring[3 * F * RS];
  __shared__ __attribute__((aligned(16))) float pst[2 * F * PR];
  __shared__ double acc[2][WK_PW][UP];  // the writers' partial sums of duration and of t * posterior
  __shared__ int lab_s[UP];

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int blank = p.blank, dt = p.xdtype, U = p.U;
  const bool lpin = p.wrt != 0;
  const int Tb = frame_count(p, b);
  const int L = label_count(p, b);
  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  float *const po = out.post + (size_t)b * p.T * U;
  float *const bo = out.blk + (size_t)b * p.T;
  const bool want = out.dur != nullptr;

  const double lP = ws.logp[b];
  const bool feasible = lP > NINF && lP < -NINF;  // (then L <= U <= UP)
  // Every element has a writer.  Padded frames are zero; an utterance without a lattice to sweep is written here as a whole: zeros
  // and -1 for an infeasible one or one without frames, and without labels every frame is the blank's, exactly
  const bool sweep = feasible && Tb > 0 && L > 0;
  const int Tz = sweep ? Tb : 0;
  for (size_t q = (size_t)Tz * U + tid; q < (size_t)p.T * U; q += WK_BWD_THREADS) po[q] = 0.f;
  for (int t = Tz + tid; t < p.T; t += WK_BWD_THREADS) bo[t] = (feasible && t < Tb) ? 1.f : 0.f;  // (t < Tb: only without a sweep)
  if (!sweep) {  // (the same verdict in every wavefront: nobody waits at a barrier)
    if (want)
      for (int i = tid; i < U; i += WK_BWD_THREADS) {
        out.dur[(size_t)b * U + i] = 0.f;
        out.exf[(size_t)b * U + i] = -1.f;
      }
    return;
  }

  wk_labels<UP, WK_BWD_THREADS, OPT>(p, b, L, tid, lab_s);
  __syncthreads();

  // (the kernels without OPT and XN set their masks in the statements they always had and keep their code)
  [[maybe_unused]] WkLane<NL> ln = {};
  int lab[NL];
  unsigned wild = 0, allow = 0;
  if constexpr (OPT || XN) {
    ln = wk_lane_of<KIND, NL, OPT, XN>(lab_s, lane, L);
    wild = ln.wild;
    allow = ln.allow;
  }
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int i = lane * NL + j;
    lab[j] = lab_s[i];
    if constexpr (!(OPT || XN)) {
      if (lab[j] == WILD_LOSS_WILDCARD) wild |= 1u << j;
      if (KIND == 0 && i > 0) {
        const int q = lab_s[i - 1];
        if (lab[j] != q || lab[j] == WILD_LOSS_WILDCARD || q == WILD_LOSS_WILDCARD) allow |= 1u << j;
      }
    }
  }
  const int allow_nx = KIND == 0 ? fused::from_next_lane_i((int)(allow & 1u), 0) : 0;
  [[maybe_unused]] const unsigned skip = ln.skip, skipo = ln.skipo;
  const bool excl = XN && ln.excl;

  const int K = (Tb + F - 1) / F;       // blocks of the utterance
  const int nck = (p.T + F - 1) / F;    // checkpoint rows per utterance
  auto frames_of = [&](int kb) { return Tb - kb * F < F ? Tb - kb * F : F; };

  // ---- producers, first job: the emissions of block kb into its ring buffer, its statistics from the workspace ----
  auto gather = [&](int kb) {
    const int pw = wave - 2, t0 = kb * F;
    float *const rb = ring + (kb % 3) * F * RS;
    for (int f0 = pw * FPW; f0 < (pw + 1) * FPW; f0 += G) {
      if (t0 + f0 >= Tb) break;
      float e[G][NL];
      float4 sv[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int q = t0 + f0 + g, t = q < Tb ? q : Tb - 1;  // past the utterance's end its last frame: never stored
        const char *const row = xb + (size_t)((long)t * p.xst) * esz;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          const int tk = XN && lab[j] < 0 ? ln.nx[j] : lab[j];  // XN: a wildcard position gathers the token it excludes
          const float v = row_load1(row, tk >= 0 ? tk : blank, dt);
          e[g][j] = tk >= 0 ? v : -__builtin_inff();
        }
        sv[g] = *reinterpret_cast<const float4 *>(ws.stat + ((size_t)b * p.T + t) * 4);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (t0 + f0 + g < Tb) {
          float *const r = rb + (f0 + g) * RS;
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            float v = e[g][j];
            if constexpr (XN) {  // the alpha sweep's slot from its statistics: (max, log2(rest + 1), rest) in .y, .z, .w
              if (excl && ((wild >> j) & 1u)) v = ln.nx[j] >= 0 ? wk_log2_rest(v, sv[g].y, sv[g].w, sv[g].z) : 0.f;
            }
            r[lane * NL + j] = v;
          }
          if (lane == 0) *reinterpret_cast<float4 *>(r + UP) = sv[g];
        }
      }
    }
  };

  // ---- producers, second job: the posterior writer of block kb.  Wavefront pw takes frames pw, pw + 4, ..; a lane takes positions
  // lane, lane + 64, ..: a frame's U floats leave as one contiguous run, its blank shares meet in the wavefront in a fixed order,
  // and the lane adds what it just wrote to its float64 sums: over the frames t = pw (mod 4) of the utterance, last block first ----
  double dsum[NL], msum[NL];
#pragma unroll
  for (int q = 0; q < NL; ++q) dsum[q] = msum[q] = 0.0;
  auto writer = [&](int kb) {
    const int pw = wave - 2, nf = frames_of(kb);
    for (int f = pw; f < nf; f += WK_PW) {
      const int t = kb * F + f;
      const float *const pr = pst + ((kb & 1) * F + f) * PR;
      float *const o = po + (size_t)t * U;
      float bs = lane == 0 ? pr[2 * UP] : 0.f;
#pragma unroll
      for (int q = 0; q < NL; ++q) {
        const int i = lane + 64 * q;
        const float v = i < L ? pr[i] : 0.f;  // positions from L on: zeros
        if (i < U) o[i] = v;
        if (i < L) bs += pr[UP + i];
        if (want) {
          dsum[q] += (double)v;
          msum[q] += (double)t * (double)v;
        }
      }
      bs = wave_sum(bs);
      if (lane == 0) bo[t] = bs;
    }
  };

  // ---- recompute wave: alpha over block kb from its checkpoint, every frame's row into the block's LDS row buffer ----
  auto recompute = [&](int kb) {
    const double *const r = ws.ck + ((size_t)b * nck + kb) * SRD;
    double O[NL], C[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      if (KIND == 0) {
        const double2 v = *reinterpret_cast<const double2 *>(r + lane * NS + 2 * j);
        O[j] = v.x; C[j] = v.y;
      } else {
        O[j] = NINF; C[j] = r[lane * NS + j];
      }
    }
    double cs = r[SRD - 2];
    const int nf = frames_of(kb);
    const float *const rb = ring + (kb % 3) * F * RS;
    double *const ab = arow + (size_t)(kb & 1) * F * SRD;
    for (int f = 0; f < nf; ++f) {
      const float *const rr = rb + f * RS;
      double *const a = ab + f * SRD;
      float e[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) e[j] = rr[lane * NL + j];
      const WkFrame fr = wk_frame_of(*reinterpret_cast<const float4 *>(rr + UP), lpin, w2);
      if (KIND == 1) {  // the state BEFORE the frame
#pragma unroll
        for (int j = 0; j < NL; ++j) a[lane * NS + j] = C[j];
        if (lane == 0) a[SRD - 2] = cs;
      }
      if constexpr (OPT || XN) wk_star_step<KIND, NL, OPT, XN>(O, C, cs, e, fr, wild, allow, ln.skip, ln.skipo, excl);
      else wk_alpha_step<KIND, NL>(O, C, cs, e, fr, wild, allow);
      if (KIND == 0) {  // the state AFTER the frame
#pragma unroll
        for (int j = 0; j < NL; ++j) *reinterpret_cast<double2 *>(a + lane * NS + 2 * j) = make_double2(O[j], C[j]);
        if (lane == 0) a[SRD - 2] = cs;
      }
    }
  };

  // ---- beta wave: the posteriors of block kb's frames, last first, and beta back over each; wild_loss_kernel's MODE 3 split: the
  // labels' shares and the blank's in two planes of the block's LDS posterior rows, nothing summed here ----
  double bO[NL], bC[NL];  // beta: the mass of the frames still to come; behind the last frame only the end states have any
#pragma unroll
  for (int j = 0; j < NL; ++j) bO[j] = bC[j] = (lane * NL + j == L - 1 || (OPT && ln.last_opt && lane * NL + j == L - 2)) ? 0.0 : NINF;
  double bcs = (OPT && ln.last_opt && L == 1) ? 0.0 : NINF;  // (L > 0; OPT: a lone optional position makes the start state an end state)
  auto post = [&](double l2) { return fexp2((float)(l2 - lP)); };
  auto beta_block = [&](int kb) {
    const int nf = frames_of(kb);
    const float *const rb = ring + (kb % 3) * F * RS;
    const double *const ab = arow + (size_t)(kb & 1) * F * SRD;
    float *const pb = pst + (size_t)(kb & 1) * F * PR;
    double An[NS], Acsn;
    auto load_row = [&](int f) {
      const double *const a = ab + f * SRD;
#pragma unroll
      for (int q = 0; q < NS; ++q) An[q] = a[lane * NS + q];
      Acsn = a[SRD - 2];
    };
    load_row(nf - 1);
    for (int f = nf - 1; f >= 0; --f) {
      const float *const rr = rb + f * RS;
      float *const o = pb + f * PR;
      float e[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) e[j] = rr[lane * NL + j];
      const WkFrame fr = wk_frame_of(*reinterpret_cast<const float4 *>(rr + UP), lpin, w2);
      const double eb = fr.eb;
      // (XN, in an utterance that excludes: the ring slot of a wildcard position is log2(1 - p_t(y)))
      auto ewj = [&](int j) { return excl ? fr.ew + (double)e[j] : fr.ew; };
      auto em = [&](int j) { return ((wild >> j) & 1u) ? ewj(j) : fma((double)e[j] - fr.Md, LOG2E_D, fr.nl2s); };
      double A[NS];
#pragma unroll
      for (int q = 0; q < NS; ++q) A[q] = An[q];
      const double Acs = Acsn;
      if (f > 0) load_row(f - 1);  // the next frame's row, a frame ahead
      float pl[NL], pk[NL];  // the labels' shares of the lane's positions and the blank's
      if (KIND == 0) {  // the open states are the labels', the closed ones and the start state the blank's
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          pl[j] = post(A[2 * j] + bO[j]);
          pk[j] = post(A[2 * j + 1] + bC[j]);
        }
        wk_put_run<NL>(o + lane * NL, pl);
        wk_put_run<NL>(o + UP + lane * NL, pk);
        if (lane == 0) o[2 * UP] = post(Acs + bcs);
        double x = bO[0] + em(0);
        const double xl = from_next_lane(x, NINF);
        if constexpr (OPT) {  // the mirror image of wk_star_step, as in wild_ckpt_bwd_kernel: one and two positions ahead
          double x1 = NL > 1 ? bO[NL > 1 ? 1 : 0] + em(NL > 1 ? 1 : 0) : xl;
          const double xl2 = from_next_lane(x1, NINF);
          bcs = wk_lse(bcs + eb, x, ((skip >> 1) & 1u) ? x1 : NINF);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double x2 = j + 2 < NL ? bO[j + 2 < NL ? j + 2 : 0] + em(j + 2 < NL ? j + 2 : 0) : j + 2 == NL ? xl : xl2;
            const bool al = j + 1 < NL ? ((allow >> (j + 1)) & 1u) != 0 : allow_nx != 0;
            const double cb = bC[j] + eb;
            bO[j] = wk_lse(x, cb, al ? x1 : NINF, ((skipo >> (j + 2)) & 1u) ? x2 : NINF);
            bC[j] = wk_lse(cb, x1, ((skip >> (j + 2)) & 1u) ? x2 : NINF);
            x = x1;
            x1 = x2;
          }
        } else {
          bcs = wk_lse(bcs + eb, x);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double xn = j + 1 < NL ? bO[j + 1 < NL ? j + 1 : 0] + em(j + 1 < NL ? j + 1 : 0) : xl;
            const bool al = j + 1 < NL ? ((allow >> (j + 1)) & 1u) != 0 : allow_nx != 0;
            const double cb = bC[j] + eb;
            bO[j] = wk_lse(x, cb, al ? xn : NINF);
            bC[j] = wk_lse(cb, xn);
            x = xn;
          }
        }
      } else {  // entering a position is its label's; a stay emits the wildcard behind a wildcard, the blank otherwise
        const double ap0 = from_prev_lane(A[NL - 1], Acs);
        [[maybe_unused]] double ap00 = NINF;  // OPT: alpha two positions before the lane's first
        if constexpr (OPT) ap00 = from_prev_lane(NL == 1 ? ap0 : A[NL > 1 ? NL - 2 : 0], NINF);
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          double ap = j > 0 ? A[j > 0 ? j - 1 : 0] : ap0;
          if constexpr (OPT) {  // entered from one position back or, over a skipped star, from two: the frame is the position's
            const double ap2 = j > 1 ? A[j > 1 ? j - 2 : 0] : j == 1 ? ap0 : ap00;
            ap = wk_lse(ap, ((skip >> j) & 1u) ? ap2 : NINF);
          }
          const bool wj = ((wild >> j) & 1u) != 0;
          const float pe = post(ap + em(j) + bC[j]), ps = post(A[j] + (wj ? ewj(j) : eb) + bC[j]);
          pl[j] = wj ? pe + ps : pe;
          pk[j] = wj ? 0.f : ps;
        }
        wk_put_run<NL>(o + lane * NL, pl);
        wk_put_run<NL>(o + UP + lane * NL, pk);
        if (lane == 0) o[2 * UP] = post(Acs + eb + bcs);
        double x = bC[0] + em(0);
        const double xl = from_next_lane(x, NINF);
        if constexpr (OPT) {
          double x1 = NL > 1 ? bC[NL > 1 ? 1 : 0] + em(NL > 1 ? 1 : 0) : xl;
          const double xl2 = from_next_lane(x1, NINF);
          bcs = wk_lse(bcs + eb, x, ((skip >> 1) & 1u) ? x1 : NINF);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double x2 = j + 2 < NL ? bC[j + 2 < NL ? j + 2 : 0] + em(j + 2 < NL ? j + 2 : 0) : j + 2 == NL ? xl : xl2;
            bC[j] = wk_lse(bC[j] + (((wild >> j) & 1u) ? ewj(j) : eb), x1, ((skip >> (j + 2)) & 1u) ? x2 : NINF);
            x1 = x2;
          }
        } else {
          bcs = wk_lse(bcs + eb, x);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double xn = j + 1 < NL ? bC[j + 1 < NL ? j + 1 : 0] + em(j + 1 < NL ? j + 1 : 0) : xl;
            bC[j] = wk_lse(bC[j] + (((wild >> j) & 1u) ? ewj(j) : eb), xn);
            x = xn;
          }
        }
      }
    }
  };

  // every wavefront derives the same K from T_b: K + 3 barriers each, by construction
  for (int s = 0; s <= K + 2; ++s) {
    if (wave == 0) {
      const int kb = K + 1 - s;
      if (kb >= 0 && kb < K) beta_block(kb);
    } else if (wave == 1) {
      const int kb = K - s;
      if (kb >= 0 && kb < K) recompute(kb);
    } else {
      const int kg = K - 1 - s, kr = K + 2 - s;
      if (kg >= 0) gather(kg);
      if (kr >= 0 && kr < K) writer(kr);
    }
    fused::block_barrier();
  }

  if (!want) return;  // (the same in every thread)
  // the four writers' sums meet in LDS and are added in the order of the wavefronts; the quotient in float64, rounded once
  if (wave >= 2) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      acc[0][wave - 2][lane + 64 * q] = dsum[q];
      acc[1][wave - 2][lane + 64 * q] = msum[q];
    }
  }
  __syncthreads();
  if (tid < U) {
    double d = 0.0, m = 0.0;
#pragma unroll
    for (int pw = 0; pw < WK_PW; ++pw) { d += acc[0][pw][tid]; m += acc[1][pw][tid]; }
    out.dur[(size_t)b * U + tid] = (float)d;
    out.exf[(size_t)b * U + tid] = d > 0.0 ? (float)(m / d) : -1.f;  // (positions from L on summed zeros)
  }
}

template <int KIND, int NL, bool OPT, bool XN>
hipError_t launch_wild_ckpt_post(const Problem &p, double w2, float *loss, const WkWs &ws, const WkPost &out, hipStream_t st) {
  hipLaunchKernelGGL((wild_ckpt_fwd_kernel<KIND, NL, OPT, XN>), dim3(p.B), dim3(WK_FWD_THREADS), 0, st, p, w2, loss, ws);
  if (hipError_t e = hipGetLastError()) return e;
  // (T == 0 or U == 0 too: the statistics of such a call are written by the same kernel)
  hipLaunchKernelGGL((wild_ckpt_post_kernel<KIND, NL, OPT, XN>), dim3(p.B), dim3(WK_BWD_THREADS), 0, st, p, w2, ws, out);
  return hipGetLastError();
}

template <int KIND, int NL, bool OPT, bool XN>
hipError_t launch_wild_ckpt(const Problem &p, double w2, const float *d_loss, float *loss, void *grad, const WkWs &ws, hipStream_t st) {
  hipLaunchKernelGGL((wild_ckpt_fwd_kernel<KIND, NL, OPT, XN>), dim3(p.B), dim3(WK_FWD_THREADS), 0, st, p, w2, loss, ws);
  if (hipError_t e = hipGetLastError()) return e;
  if (p.T == 0) return hipSuccess;  // no rows
  hipLaunchKernelGGL((wild_ckpt_bwd_kernel<KIND, NL, OPT, XN>), dim3(p.B), dim3(WK_BWD_THREADS), 0, st, p, w2, d_loss, ws, grad);
  return hipGetLastError();
}

inline size_t wk_al(size_t x) { return (x + 255) & ~size_t(255); }
inline bool wk_tier(int U) { return U <= WILD_CKPT_MAX_U; }
inline size_t wk_ck_bytes(int kind, int B, int T, int U) {
  const int NL = nl_for(U), F = wild_ckpt_frames(NL);
  return (size_t)B * ((T + F - 1) / F) * wk_row_doubles(kind, 64 * NL) * 8;
}
inline WkWs wk_regions(const Problem &p, char *wsp) {
  const size_t ck = wk_al(wk_ck_bytes(p.kind, p.B, p.T, p.U));
  return WkWs{reinterpret_cast<double *>(wsp), reinterpret_cast<float *>(wsp + ck),
              reinterpret_cast<double *>(wsp + ck + wk_al((size_t)p.B * p.T * 16))};
}

// the two launches of one (OPT, XN) on a workspace of wild_loss_ckpt_workspace_bytes(want_grad = true): grad != nullptr, U <= 256
template <bool OPT, bool XN>
hipError_t wk_run(const Problem &p, float wildcard_log_weight, const float *d_loss, float *loss, void *grad, char *wsp, hipStream_t st) {
  typedef hipError_t Launch(const Problem &, double, const float *, float *, void *, const WkWs &, hipStream_t);
  static Launch *const table[2][3] = {{launch_wild_ckpt<0, 1, OPT, XN>, launch_wild_ckpt<0, 2, OPT, XN>, launch_wild_ckpt<0, 4, OPT, XN>},
                                      {launch_wild_ckpt<1, 1, OPT, XN>, launch_wild_ckpt<1, 2, OPT, XN>, launch_wild_ckpt<1, 4, OPT, XN>}};
  const int NL = nl_for(p.U);
  if (p.kind < 0 || p.kind > 1 || NL > 4) return hipErrorInvalidValue;
  return table[p.kind][NL == 1 ? 0 : NL == 2 ? 1 : 2](p, (double)wildcard_log_weight * LOG2E_D, d_loss, loss, grad, wk_regions(p, wsp), st);
}

// ... and of the label posteriors on the same workspace: U <= 256
template <bool OPT, bool XN>
hipError_t wk_post_run(const Problem &p, float wildcard_log_weight, float *loss, const WkPost &out, char *wsp, hipStream_t st) {
  typedef hipError_t Launch(const Problem &, double, float *, const WkWs &, const WkPost &, hipStream_t);
  static Launch *const table[2][3] = {
      {launch_wild_ckpt_post<0, 1, OPT, XN>, launch_wild_ckpt_post<0, 2, OPT, XN>, launch_wild_ckpt_post<0, 4, OPT, XN>},
      {launch_wild_ckpt_post<1, 1, OPT, XN>, launch_wild_ckpt_post<1, 2, OPT, XN>, launch_wild_ckpt_post<1, 4, OPT, XN>}};
  const int NL = nl_for(p.U);
  if (p.kind < 0 || p.kind > 1 || NL > 4) return hipErrorInvalidValue;
  return table[p.kind][NL == 1 ? 0 : NL == 2 ? 1 : 2](p, (double)wildcard_log_weight * LOG2E_D, loss, wk_regions(p, wsp), out, st);
}

}  // namespace

#if defined(CTC_CKPT_OPT)
hipError_t run_wild_loss_ckpt_opt(const Problem &p, float wildcard_log_weight, const float *d_loss, float *loss, void *grad, char *wsp,
                                  hipStream_t st) {
  return wk_run<true, false>(p, wildcard_log_weight, d_loss, loss, grad, wsp, st);
}
hipError_t run_label_posterior_ckpt_opt(const Problem &p, float wildcard_log_weight, float *loss, float *label_posterior,
                                        float *blank_posterior, float *duration, float *expected_frame, char *wsp, hipStream_t st) {
  return wk_post_run<true, false>(p, wildcard_log_weight, loss, WkPost{label_posterior, blank_posterior, duration, expected_frame}, wsp, st);
}
#elif defined(CTC_STAR)
hipError_t run_wild_loss_ckpt_star(const Problem &p, float wildcard_log_weight, const float *d_loss, float *loss, void *grad, char *wsp,
                                   hipStream_t st, bool optional_wildcards) {
  return optional_wildcards ? wk_run<true, true>(p, wildcard_log_weight, d_loss, loss, grad, wsp, st)
                            : wk_run<false, true>(p, wildcard_log_weight, d_loss, loss, grad, wsp, st);
}
hipError_t run_label_posterior_ckpt_star(const Problem &p, float wildcard_log_weight, float *loss, float *label_posterior,
                                         float *blank_posterior, float *duration, float *expected_frame, char *wsp, hipStream_t st,
                                         bool optional_wildcards) {
  const WkPost out{label_posterior, blank_posterior, duration, expected_frame};
  return optional_wildcards ? wk_post_run<true, true>(p, wildcard_log_weight, loss, out, wsp, st)
                            : wk_post_run<false, true>(p, wildcard_log_weight, loss, out, wsp, st);
}
#else
// checkpoints, then the row statistics, then log2 Z: each region rounded up to 256 bytes (include/ctc_amd.h has the formula)
size_t wild_loss_ckpt_workspace_bytes(int kind, int B, int T, int U, bool want_grad) {
  if (!want_grad) return 0;
  if (!wk_tier(U)) return wild_loss_workspace_bytes(kind, B, T, U, true);
  return wk_al(wk_ck_bytes(kind, B, T, U)) + wk_al((size_t)B * T * 16) + wk_al((size_t)B * 8);
}

hipError_t run_wild_loss_ckpt(const Problem &p, float wildcard_log_weight, const float *d_loss, float *loss, void *grad, char *wsp,
                              hipStream_t st) {
  if (!grad || !wk_tier(p.U)) return run_wild_loss(p, wildcard_log_weight, d_loss, loss, grad, wsp, st);
  return wk_run<false, false>(p, wildcard_log_weight, d_loss, loss, grad, wsp, st);
}

hipError_t run_star_loss_ckpt(const Problem &p, float wildcard_log_weight, const float *d_loss, float *loss, void *grad, char *wsp,
                              hipStream_t st, bool optional_wildcards, bool exclude_next_label) {
  if (!grad || !wk_tier(p.U))
    return exclude_next_label ? run_star_loss(p, wildcard_log_weight, d_loss, loss, grad, wsp, st, nullptr, 0, optional_wildcards)
                              : run_wild_loss(p, wildcard_log_weight, d_loss, loss, grad, wsp, st, nullptr, 0, optional_wildcards);
  if (exclude_next_label) return run_wild_loss_ckpt_star(p, wildcard_log_weight, d_loss, loss, grad, wsp, st, optional_wildcards);
  if (optional_wildcards) return run_wild_loss_ckpt_opt(p, wildcard_log_weight, d_loss, loss, grad, wsp, st);
  return wk_run<false, false>(p, wildcard_log_weight, d_loss, loss, grad, wsp, st);
}

hipError_t run_label_posterior_ckpt(const Problem &p, float wildcard_log_weight, float *loss, float *label_posterior, float *blank_posterior,
                                    float *duration, float *expected_frame, char *wsp, hipStream_t st) {
  if (!wk_tier(p.U)) return run_label_posterior(p, wildcard_log_weight, loss, label_posterior, blank_posterior, duration, expected_frame, wsp, st);
  return wk_post_run<false, false>(p, wildcard_log_weight, loss, WkPost{label_posterior, blank_posterior, duration, expected_frame}, wsp, st);
}

hipError_t run_star_label_posterior_ckpt(const Problem &p, float wildcard_log_weight, float *loss, float *label_posterior,
                                         float *blank_posterior, float *duration, float *expected_frame, char *wsp, hipStream_t st,
                                         bool optional_wildcards, bool exclude_next_label) {
  if (!wk_tier(p.U))
    return (exclude_next_label ? run_star_label_posterior : run_label_posterior)(p, wildcard_log_weight, loss, label_posterior, blank_posterior,
                                                                                 duration, expected_frame, wsp, st, nullptr, 0,
                                                                                 optional_wildcards);
  if (exclude_next_label)
    return run_label_posterior_ckpt_star(p, wildcard_log_weight, loss, label_posterior, blank_posterior, duration, expected_frame, wsp, st,
                                         optional_wildcards);
  if (optional_wildcards)
    return run_label_posterior_ckpt_opt(p, wildcard_log_weight, loss, label_posterior, blank_posterior, duration, expected_frame, wsp, st);
  return run_label_posterior_ckpt(p, wildcard_log_weight, loss, label_posterior, blank_posterior, duration, expected_frame, wsp, st);
}
#endif

}  // namespace ctc
