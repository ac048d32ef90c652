// CTC loss and gradient with wildcard labels (W-CTC / star CTC) on both lattices: ctc_amd_wildcard_loss_grad (include/ctc_amd.h),
// DESIGN.md section 5.16.  The training-side counterpart of ctc_align_wild.hip: the same lattice, summed over all its paths.
//
// The decomposition of ctc_nbest.hip for ONE transcript per utterance (its file-local helpers are repeated here; that file stays as
// it is).  One workgroup per utterance, five wavefronts:
//   wave 0      the chain: NL label positions per lane (position i = lane * NL + j), neighbours by DPP, the state in registers as
//               float64 base-2 logarithms with a true -inf as log(0): nothing is rescaled, nothing can be flushed;
//   waves 1..4  producers, one block of frames ahead through an LDS ring: each lane gathers x[t, label[i]] of its own NL positions
//               and the wavefront streams the row once for (max, sum of exp).  No V-wide row is staged in LDS: any V costs no LDS.
// A label equal to WILD_LOSS_WILDCARD marks a wildcard position.  Its emission is the wave-uniform e_w(t) = w + ln sum_k exp(lp[t, k]):
// the constant w for logits, w plus the row's log-sum-exp for log-probabilities.  What differs from the plain recursion:
//     O'[i] = lse(O[i], C[i-1], O[i-1] if label[i] != label[i-1] or either is a wildcard) + e[i]     e[i] = e_w for a wildcard
//     C'[i] = lse(C[i], O[i]) + e[blank]
//     S'[i] = lse(S[i] + (e_w if i is a wildcard else e[blank]), S[i-1] + e[i])
// -- classic: two more sources of the `allow` bits, set once; simplified: one select per position for the horizontal weight.
//
// The kernel body runs in four modes (template parameter MODE), the first three as ctc_nbest.hip's:
//   MODE 0  the loss alone;
//   MODE 1  the same alpha sweep, bit for bit, that also stores the chain's state of every frame (float64), log2 Z and the row
//           statistics to the workspace;
//   MODE 2  the beta sweep, frames from T_b - 1 down: per frame the chain reads its saved row, forms the posteriors
//           2^(alpha + beta - log2 Z) and writes them as float32 pairs over the slots it has just read, then steps beta back;
//   MODE 3  the beta sweep of ctc_amd_label_posterior: the same recursion and the same posteriors, but the
//           saved rows stay as they are; each label position's posterior goes straight to label_posterior[b, t, i] (a lane's NL
//           positions are contiguous: a frame is one run of U floats) and the blank's share, summed over the wavefront in a fixed
//           order, to blank_posterior[b, t].  Rows t >= T_b and whole infeasible utterances are zeroed by the same workgroup;
//   label_stat_kernel  duration and expected_frame: one lane per label position, float64 sums over the frames of the matrix
//           MODE 3 has just written;
//   wild_grad_row_kernel  one wavefront per row (b, t): the posteriors of ordinary positions go into 64-bit fixed-point LDS bins by
//           token (integer atomics: no arrival order in the sum), those of wildcard positions and of the blank into per-lane sums
//           in a fixed order; the vocabulary in passes of 1024 columns; the row streams out as d_loss * (c * softmax - bins) with
//           c = 1 - Gamma_t (logits) or -Gamma_t (log-probabilities; softmax is then exp(x - LSE_t)).
// WIN (ctc_amd_windowed_loss_grad / _label_posterior): every lane holds the (first, last) frames of its own
// NL positions; the producers write -inf for an ordinary position whose frame lies outside them and, into the ring slot of a wildcard
// position (which holds -inf otherwise and is never read), the gate 0 / -inf that the chain adds to the wave-uniform e_w.  The row
// stage and the statistics know nothing of windows.
// OPT (ctc_amd_optional_wildcard_loss_grad / _label_posterior): a label equal to WILD_LOSS_OPTIONAL is a
// wildcard position that may be skipped.  Two mask bits per position, set once (`skip`: the position before me is optional; `skipo`:
// classic, the open -> open step over it is allowed), add to the recursions above
//     O'[i] += C[i-2] if skip, O[i-2] if skipo          S'[i] += S[i-2] + e[i] if skip          (position -1 is the start state)
// with the state two positions back taken from the lane's own registers or by one more DPP shift, and the beta sweep the mirror
// image; a last optional position makes the states before it end states.  The further terms come behind the existing ones in the
// sums: -inf there leaves the bits as they are.  The row stage counts the optional wildcard as a wildcard; nothing else knows of it.
// A saved row of frame t: per position i the pair (O, C) (classic, AFTER frame t) or S (simplified, BEFORE frame t), then the start
// state: (2 or 1) * UP + 2 doubles.  After the beta sweep the first 8 bytes of position i hold
//   classic:    (posterior of O[i] after frame t,  posterior of C[i] = a blank behind label i)
//   simplified: (posterior of entering i at t,     posterior of staying in S[i] at t)
// and the start state's slot its blank posterior.  .x belongs to the token's column, or to Gamma_t for a wildcard; .y to the blank's
// column, or (simplified, behind a wildcard) to Gamma_t.
#include "ctc_wild_loss.h"

#include <type_traits>

namespace ctc {
namespace {

constexpr int WL_PW = 4;                      // producer wavefronts
constexpr int WL_THREADS = 64 * (1 + WL_PW);  // + the chain
constexpr int WL_RING = 4096;                 // label emissions per ring buffer (two buffers): frames per block = 4096 / UP
constexpr double LOG2E_D = 1.44269504088896340736;

__device__ __forceinline__ float4 wl_row_load4(const char *row, int k, int dt) {
  if (dt == 0) return *reinterpret_cast<const float4 *>(row + (size_t)k * 4);
  const uint2 u = *reinterpret_cast<const uint2 *>(row + (size_t)k * 2);
  return make_float4(h16_to_f32((unsigned short)(u.x & 0xffffu), dt), h16_to_f32((unsigned short)(u.x >> 16), dt),
                     h16_to_f32((unsigned short)(u.y & 0xffffu), dt), h16_to_f32((unsigned short)(u.y >> 16), dt));
}
// the same four elements one by one (unaligned rows, V no multiple of 4): -inf past the row, which adds nothing to either statistic
__device__ __forceinline__ float4 wl_row_load4_elem(const char *row, int k, int V, int dt) {
  const float ninf = -__builtin_inff();
  return make_float4(row_load1(row, k, dt), k + 1 < V ? row_load1(row, k + 1, dt) : ninf, k + 2 < V ? row_load1(row, k + 2, dt) : ninf,
                     k + 3 < V ? row_load1(row, k + 3, dt) : ninf);
}
// running (max, sum of exp(x - max)) of one lane: four more elements (both access paths end here: identical bits)
__device__ __forceinline__ void wl_stat_add4(float &m, float &s, const float4 v) {
  const float mn = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
  s = s * fexp2((m - mn) * LOG2E) +
      ((fexp2((v.x - mn) * LOG2E) + fexp2((v.y - mn) * LOG2E)) + (fexp2((v.z - mn) * LOG2E) + fexp2((v.w - mn) * LOG2E)));
  m = mn;
}

// base-2 log(2^a + 2^b [+ 2^c]) of float64 operands that may be -inf (log 0): differences against the maximum, or against 0
// when every operand is -inf (then every term is exp2(-inf) = 0 and the result log2(0) = -inf, without a NaN on the way)
__device__ __forceinline__ double wl_lse(double a, double b) {
  const double m = fmax(a, b);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2(fexp2((float)(a - mm)) + fexp2((float)(b - mm)));
}
__device__ __forceinline__ double wl_lse(double a, double b, double c) {
  const double m = fmax(fmax(a, b), c);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2((fexp2((float)(a - mm)) + fexp2((float)(b - mm))) + fexp2((float)(c - mm)));
}

// ... four and five operands (OPT): the further terms are added behind the first three, so operands of -inf there leave the bits
// of the three-operand result as they are
__device__ __forceinline__ double wl_lse(double a, double b, double c, double d) {
  const double m = fmax(fmax(a, b), fmax(c, d));
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2(((fexp2((float)(a - mm)) + fexp2((float)(b - mm))) + fexp2((float)(c - mm))) + fexp2((float)(d - mm)));
}
__device__ __forceinline__ double wl_lse(double a, double b, double c, double d, double e) {
  const double m = fmax(fmax(fmax(a, b), fmax(c, d)), e);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2((((fexp2((float)(a - mm)) + fexp2((float)(b - mm))) + fexp2((float)(c - mm))) + fexp2((float)(d - mm))) +
                            fexp2((float)(e - mm)));
}

// the gradient's workspace (MODE 0: unused)
struct WlWs {
  double *rows;  // [B][T][SRD] saved alpha rows, then the posteriors
  float *stat;   // [B][T][4] x[blank], row max, log2 sum exp(x - max) of every frame
  double *logp;  // [B] log2 Z, -inf for an infeasible utterance
};
constexpr int wl_row_doubles(int kind, int UP) { return (kind == 0 ? 2 : 1) * UP + 2; }
// ... and what MODE 3 writes instead of the posteriors in the rows
struct WlPostWs : WlWs {
  float *post;  // [B][T][U] label_posterior
  float *blk;   // [B][T] blank_posterior
};
template <int MODE> using WlArg = std::conditional_t<MODE == 3, WlPostWs, WlWs>;

template <int KIND, int NL, int MODE, bool WIN, bool OPT>
__global__ __launch_bounds__(WL_THREADS) void wild_loss_kernel(const Problem p, const double w2, float *__restrict__ loss,
                                                               const WlArg<MODE> ws, const int32_t *__restrict__ win, int wstride) {
  static_assert(!(WIN && OPT), "frame windows and optional wildcards are not combined");
  constexpr bool BACK = MODE >= 2;              // a beta sweep: frames from T_b - 1 down
  constexpr int UP = 64 * NL;
  constexpr int NS = (KIND == 0 ? 2 : 1) * NL;  // doubles of a saved row per lane
  constexpr int SRD = wl_row_doubles(KIND, UP);
  constexpr bool PF = NL <= 4;                  // beta sweeps: the next frame's saved row is requested one frame ahead
  constexpr int F = WL_RING / UP;               // frames per ring buffer: 64, 32, 16, 8, 4
  constexpr int RS = UP + 4;                    // ring row: UP label emissions, then x[blank], the row max, log2 sum exp(x - max)
  constexpr int FPW = F / WL_PW;                // frames per producer wavefront and block
  constexpr int G = FPW < 4 ? FPW : 4;          // ... of which G are in flight together
  const double NINF = -__builtin_inf();

  __shared__ __attribute__((aligned(16))) float ring[2 * F * RS];
  __shared__ int lab_s[UP];  // validated labels (-1: no emission, WILD_LOSS_WILDCARD: a wildcard)

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int V = p.V, blank = p.blank, dt = p.xdtype;
  const bool lpin = p.wrt != 0;  // log-probability input
  const int Tb = frame_count(p, b);
  int L = label_count(p, b);
  const bool too_long = too_many_labels(p, L);
  if (too_long) L = 0;  // (nothing of such an utterance is read; it is reported infeasible below)

  double lP = 0.0;
  if constexpr (BACK) lP = ws.logp[b];
  const bool feasible = lP > NINF && lP < -NINF;  // (the same in every thread)
  if constexpr (MODE == 3) {  // every element has a writer: frames from T_b on, and every frame of an infeasible utterance, are zero
    const size_t z0 = (size_t)(feasible ? Tb : 0), nz = (size_t)p.T - z0;
    float *const zp = ws.post + ((size_t)b * p.T + z0) * p.U;
    for (size_t q = tid; q < nz * p.U; q += WL_THREADS) zp[q] = 0.f;
    float *const zb = ws.blk + (size_t)b * p.T + z0;
    for (size_t q = tid; q < nz; q += WL_THREADS) zb[q] = 0.f;
  }
  // an infeasible utterance has no posteriors: the row stage (MODE 2) writes its zeros without them
  if (BACK && !feasible) return;

  for (int i = tid; i < UP; i += WL_THREADS) {
    int tok = -1;
    if (i < L) tok = label_at(p, label_row(p, b), i);
    int cls = tok == WILD_LOSS_WILDCARD ? WILD_LOSS_WILDCARD : emits(p, tok) ? tok : -1;
    if constexpr (OPT) {  // an optional wildcard; beside another one it is a bad label: no emission, no skip
      if (tok == WILD_LOSS_OPTIONAL) {
        const int32_t *const lr = label_row(p, b);
        const bool pair = (i > 0 && label_at(p, lr, i - 1) == WILD_LOSS_OPTIONAL) || (i + 1 < L && label_at(p, lr, i + 1) == WILD_LOSS_OPTIONAL);
        cls = pair ? -1 : WILD_LOSS_OPTIONAL;
      }
    }
    lab_s[i] = cls;
  }
  __syncthreads();

  auto is_wild = [](int tok) { return tok == WILD_LOSS_WILDCARD || (OPT && tok == WILD_LOSS_OPTIONAL); };
  int lab[NL];
  unsigned wild = 0;  // bit j = position lane * NL + j is a wildcard (OPT: of either kind)
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    lab[j] = lab_s[lane * NL + j];
    if (is_wild(lab[j])) wild |= 1u << j;
  }
  [[maybe_unused]] int wf[NL], wl[NL];  // WIN: the frames position lane * NL + j may own (from label_length on: never read, empty)
  if constexpr (WIN) {
    const int32_t *const wb = win + (size_t)b * wstride;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int i = lane * NL + j;
      wf[j] = i < L ? wb[2 * i] : 0;
      wl[j] = i < L ? wb[2 * i + 1] : -1;
    }
  }

  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  // vector row accesses (16 bytes of float32, 8 bytes of 16-bit elements) need aligned rows; element-wise otherwise
  const bool vec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (dt == 0 ? 15 : 7)) == 0;
  double *const myrows = MODE != 0 ? ws.rows + (size_t)b * p.T * SRD : nullptr;

  // ---- chain state (wave 0) ----
  double O[NL], C[NL];  // simplified: C is S, O unused.  MODE 2: beta, the mass of the frames still to come
  unsigned allow = 0;   // classic: bit j = label[i] differs from label[i-1], or one of the two is a wildcard
  int allow_nx = 0;     // ... of the next lane's first position (MODE 2)
  double cs = 0.0;      // the start state: blank so far
  auto allowed = [&](int i) {
    if (i <= 0 || i >= UP) return false;
    const int a = lab_s[i], q = lab_s[i - 1];
    return a != q || is_wild(a) || is_wild(q);
  };
  // OPT: bit q of `skip` = the position before lane * NL + q is an optional wildcard, so this one may also be entered from two
  // positions back; bit q of `skipo` = (classic) ... from the open state there too.  q runs to NL + 1: the beta sweep looks two ahead
  [[maybe_unused]] unsigned skip = 0, skipo = 0;
  [[maybe_unused]] bool last_opt = false;  // the last position is optional: the states before it are end states too
  if constexpr (OPT) {
#pragma unroll
    for (int q = 0; q < NL + 2; ++q) {
      const int i = lane * NL + q;
      if (i >= 1 && i < UP && lab_s[i - 1] == WILD_LOSS_OPTIONAL) {
        skip |= 1u << q;
        if (KIND == 0 && i >= 2 && (lab_s[i] != lab_s[i - 2] || is_wild(lab_s[i]) || is_wild(lab_s[i - 2]))) skipo |= 1u << q;
      }
    }
    last_opt = L > 0 && lab_s[L - 1] == WILD_LOSS_OPTIONAL;
  }
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    O[j] = NINF; C[j] = NINF;
    if (KIND == 0 && allowed(lane * NL + j)) allow |= 1u << j;
  }
  if constexpr (BACK) {  // behind the last frame only the end states have any mass
#pragma unroll
    for (int j = 0; j < NL; ++j) O[j] = C[j] = (lane * NL + j == L - 1 || (OPT && last_opt && lane * NL + j == L - 2)) ? 0.0 : NINF;
    cs = (L == 0 || (OPT && last_opt && L == 1)) ? 0.0 : NINF;
    if (KIND == 0) allow_nx = allowed((lane + 1) * NL) ? 1 : 0;
  }

  // the frame a block's position stands for (MODE 2 runs backwards); past the utterance's end its last, valid memory whose
  // results are never stored
  auto real_t = [&](int q) {
    const int c = q < Tb ? q : Tb - 1;
    return BACK ? Tb - 1 - c : c;
  };

  auto produce = [&](int kb) {
    const int pw = wave - 1, q0 = kb * F;
    float *const rb = ring + (kb & 1) * F * RS;
    for (int f0 = pw * FPW; f0 < (pw + 1) * FPW; f0 += G) {
      if (q0 + f0 >= Tb) break;
      const char *row[G];
#pragma unroll
      for (int g = 0; g < G; ++g) row[g] = xb + (size_t)((long)real_t(q0 + f0 + g) * p.xst) * esz;
      float e[G][NL], eb[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          const float v = row_load1(row[g], lab[j] >= 0 ? lab[j] : blank, dt);
          e[g][j] = lab[j] >= 0 ? v : -__builtin_inff();
        }
        eb[g] = row_load1(row[g], blank, dt);
      }
      // the row pass.  Both access paths give a lane the same elements in the same order: identical bits
      float m[G], s[G];
#pragma unroll
      for (int g = 0; g < G; ++g) { m[g] = -3.402823466e38f; s[g] = 0.f; }
      for (int k = lane * 4; k < V; k += 256) {
        float4 v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) v[g] = vec ? wl_row_load4(row[g], k, dt) : wl_row_load4_elem(row[g], k, V, dt);
#pragma unroll
        for (int g = 0; g < G; ++g) wl_stat_add4(m[g], s[g], v[g]);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float M = wave_max(m[g]);
        const float S = wave_sum(s[g] * fexp2((m[g] - M) * LOG2E));
        float l2s = flog2(S);
        if (!(S > 0.f)) { M = 0.f; l2s = __builtin_inff(); }  // a row of -inf: every emission of the frame is -inf
        if (q0 + f0 + g < Tb) {
          float *const r = rb + (f0 + g) * RS;
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            float v = e[g][j];
            if constexpr (WIN) {
              const int t = real_t(q0 + f0 + g);
              if ((wild >> j) & 1u) v = 0.f;  // the gate of e_w
              if (t < wf[j] || t > wl[j]) v = -__builtin_inff();
            }
            r[lane * NL + j] = v;
          }
          if (lane == 0) {
            *reinterpret_cast<float4 *>(r + UP) = make_float4(eb[g], M, l2s, 0.f);
            if (MODE == 1) *reinterpret_cast<float4 *>(ws.stat + ((size_t)b * p.T + real_t(q0 + f0 + g)) * 4) = make_float4(eb[g], M, l2s, 0.f);
          }
        }
      }
    }
  };

  // what a ring row says about its frame, in the lattice's units (base-2 logarithms of lp)
  struct Frame {
    double Md, nl2s, eb, ew;
  };
  auto frame_of = [&](const float *r) {
    const float4 sv = *reinterpret_cast<const float4 *>(r + UP);
    Frame fr;
    // logits: lp = x - max - ln sum; log-probabilities: lp = x
    fr.Md = lpin ? 0.0 : (double)sv.y;
    fr.nl2s = lpin ? 0.0 : -(double)sv.z;
    fr.eb = fma((double)sv.x - fr.Md, LOG2E_D, fr.nl2s);
    // e_w = w + ln sum_k exp(lp[t, k]): w for logits, w + LSE_t for log-probabilities; a row of -inf emits nothing
    fr.ew = sv.z == __builtin_inff() ? NINF : lpin ? w2 + fma((double)sv.y, LOG2E_D, (double)sv.z) : w2;
    return fr;
  };

  auto load_row = [&](int t, double (&A)[NS], double &Acs) {
    const double *const r = myrows + (size_t)t * SRD;
#pragma unroll
    for (int q = 0; q < NS; ++q) A[q] = r[lane * NS + q];
    Acs = r[SRD - 2];
  };

  auto consume = [&](int kb) {
    const int t0 = kb * F;
    const int nf = Tb - t0 < F ? Tb - t0 : F;
    const float *const rb = ring + (kb & 1) * F * RS;
    for (int f = 0; f < nf; ++f) {
      const float *const rr = rb + f * RS;
      float e[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) e[j] = rr[lane * NL + j];
      const Frame fr = frame_of(rr);
      const double eb = fr.eb;
      auto ewj = [&](int j) { return WIN ? fr.ew + (double)e[j] : fr.ew; };  // (WIN: the ring slot of a wildcard is its gate, 0 or -inf)
      auto em = [&](int j) { return ((wild >> j) & 1u) ? ewj(j) : fma((double)e[j] - fr.Md, LOG2E_D, fr.nl2s); };
      double *const r = MODE == 1 ? myrows + (size_t)(t0 + f) * SRD : nullptr;
      if (MODE == 1 && KIND == 1) {  // the state BEFORE the frame
#pragma unroll
        for (int j = 0; j < NL; ++j) r[lane * NS + j] = C[j];
        if (lane == 0) r[SRD - 2] = cs;
      }
      if (KIND == 0) {
        const double pO = from_prev_lane(O[NL - 1], NINF);
        const double pC = from_prev_lane(C[NL - 1], cs);
        // OPT: the position two before the lane's first: the previous lane's last but one (NL = 1: two lanes back; before lane 0
        // lies the start state, and nothing before that)
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
            o = wl_lse(O[j], qC, a2, ((skip >> j) & 1u) ? rC : NINF, ((skipo >> j) & 1u) ? rO : NINF) + em(j);
          } else {
            o = wl_lse(O[j], qC, a2) + em(j);
          }
          C[j] = wl_lse(C[j], O[j]) + eb;
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
            C[j] = wl_lse(C[j] + (((wild >> j) & 1u) ? ewj(j) : eb), q + em(j), ((skip >> j) & 1u) ? r + em(j) : NINF);
          } else {
            C[j] = wl_lse(C[j] + (((wild >> j) & 1u) ? ewj(j) : eb), q + em(j));
          }
        }
      }
      cs += eb;
      if (MODE == 1 && KIND == 0) {  // the state AFTER the frame
#pragma unroll
        for (int j = 0; j < NL; ++j) *reinterpret_cast<double2 *>(r + lane * NS + 2 * j) = make_double2(O[j], C[j]);
        if (lane == 0) r[SRD - 2] = cs;
      }
    }
  };

  // MODE 3: a lane's NL label posteriors of frame t (positions from U on are not written) and its part of the blank's share.
  // Vector stores where U and the base pointer keep every group of VW positions aligned and whole, element-wise otherwise
  [[maybe_unused]] auto put_post = [&](int t, const float (&pl)[NL], float pb) {
    if constexpr (MODE == 3) {
      constexpr int VW = NL < 4 ? NL : 4;
      float *const o = ws.post + ((size_t)b * p.T + t) * p.U;
      const int i0 = lane * NL, U = p.U;
      if (p.U % VW == 0 && (reinterpret_cast<uintptr_t>(ws.post) & (VW * 4 - 1)) == 0) {
#pragma unroll
        for (int j = 0; j < NL; j += VW) {
          if (i0 + j < U) {
            if constexpr (VW == 4) *reinterpret_cast<float4 *>(o + i0 + j) = make_float4(pl[j], pl[j + 1], pl[j + 2], pl[j + 3]);
            else if constexpr (VW == 2) *reinterpret_cast<float2 *>(o + i0 + j) = make_float2(pl[j], pl[j + 1]);
            else o[i0 + j] = pl[j];
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < NL; ++j)
          if (i0 + j < U) o[i0 + j] = pl[j];
      }
      const float bs = wave_sum(pb);
      if (lane == 0) ws.blk[(size_t)b * p.T + t] = bs;
    }
  };

  // beta sweeps: block kb holds the frames T_b - 1 - kb F downwards
  double An[NS], Acsn = 0.0;
  auto consume_back = [&](int kb) {
    const int t0 = kb * F;
    const int nf = Tb - t0 < F ? Tb - t0 : F;
    const float *const rb = ring + (kb & 1) * F * RS;
    for (int f = 0; f < nf; ++f) {
      const int t = Tb - 1 - (t0 + f);
      const float *const rr = rb + f * RS;
      float e[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) e[j] = rr[lane * NL + j];
      const Frame fr = frame_of(rr);
      const double eb = fr.eb;
      auto ewj = [&](int j) { return WIN ? fr.ew + (double)e[j] : fr.ew; };  // (WIN: the ring slot of a wildcard is its gate, 0 or -inf)
      auto em = [&](int j) { return ((wild >> j) & 1u) ? ewj(j) : fma((double)e[j] - fr.Md, LOG2E_D, fr.nl2s); };
      double A[NS], Acs;
      if constexpr (PF) {
#pragma unroll
        for (int q = 0; q < NS; ++q) A[q] = An[q];
        Acs = Acsn;
        if (t > 0) load_row(t - 1, An, Acsn);
      } else {
        load_row(t, A, Acs);
      }
      [[maybe_unused]] double *const r = myrows + (size_t)t * SRD;
      auto post = [&](double l2) { return fexp2((float)(l2 - lP)); };
      if (KIND == 0) {
        if constexpr (MODE == 3) {  // the open states are the labels', the closed ones and the start state the blank's
          float pl[NL], pb = lane == 0 ? post(Acs + cs) : 0.f;
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            pl[j] = post(A[2 * j] + O[j]);
            pb += post(A[2 * j + 1] + C[j]);
          }
          put_post(t, pl, pb);
        } else {
#pragma unroll
          for (int j = 0; j < NL; ++j)
            *reinterpret_cast<float2 *>(r + lane * NS + 2 * j) = make_float2(post(A[2 * j] + O[j]), post(A[2 * j + 1] + C[j]));
          if (lane == 0) *reinterpret_cast<float *>(r + SRD - 2) = post(Acs + cs);
        }
        // beta back over frame t: x = what entering O[i] with this frame is worth
        double x = O[0] + em(0);
        const double xl = from_next_lane(x, NINF);
        if constexpr (OPT) {
          // the mirror image of the alpha step: what entering the open states one and two positions ahead is worth; beyond the
          // lane's own they are the next lane's first two (NL = 1: the next two lanes')
          double x1 = NL > 1 ? O[NL > 1 ? 1 : 0] + em(NL > 1 ? 1 : 0) : xl;
          const double xl2 = from_next_lane(x1, NINF);
          cs = wl_lse(cs + eb, x, ((skip >> 1) & 1u) ? x1 : NINF);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double x2 = j + 2 < NL ? O[j + 2 < NL ? j + 2 : 0] + em(j + 2 < NL ? j + 2 : 0) : j + 2 == NL ? xl : xl2;
            const bool al = j + 1 < NL ? ((allow >> (j + 1)) & 1u) != 0 : allow_nx != 0;
            const double cb = C[j] + eb;
            O[j] = wl_lse(x, cb, al ? x1 : NINF, ((skipo >> (j + 2)) & 1u) ? x2 : NINF);
            C[j] = wl_lse(cb, x1, ((skip >> (j + 2)) & 1u) ? x2 : NINF);
            x = x1;
            x1 = x2;
          }
        } else {
          cs = wl_lse(cs + eb, x);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double xn = j + 1 < NL ? O[j + 1 < NL ? j + 1 : 0] + em(j + 1 < NL ? j + 1 : 0) : xl;
            const bool al = j + 1 < NL ? ((allow >> (j + 1)) & 1u) != 0 : allow_nx != 0;
            const double cb = C[j] + eb;
            O[j] = wl_lse(x, cb, al ? xn : NINF);
            C[j] = wl_lse(cb, xn);
            x = xn;
          }
        }
      } else {
        const double ap0 = from_prev_lane(A[NL - 1], Acs);
        [[maybe_unused]] double ap00 = NINF;  // OPT: alpha two positions before the lane's first
        if constexpr (OPT) ap00 = from_prev_lane(NL == 1 ? ap0 : A[NL > 1 ? NL - 2 : 0], NINF);
        [[maybe_unused]] float pl[NL], pb = 0.f;
        if (MODE == 3 && lane == 0) pb = post(Acs + eb + cs);
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          double ap = j > 0 ? A[j > 0 ? j - 1 : 0] : ap0;
          if constexpr (OPT) {  // entered from one position back or, over an optional wildcard, from two
            const double ap2 = j > 1 ? A[j > 1 ? j - 2 : 0] : j == 1 ? ap0 : ap00;
            ap = wl_lse(ap, ((skip >> j) & 1u) ? ap2 : NINF);
          }
          const bool wj = ((wild >> j) & 1u) != 0;
          const double h = wj ? ewj(j) : eb;
          const float pe = post(ap + em(j) + C[j]), ps = post(A[j] + h + C[j]);
          if constexpr (MODE == 3) {  // a stay emits the wildcard behind a wildcard, the blank otherwise
            pl[j] = wj ? pe + ps : pe;
            pb += wj ? 0.f : ps;
          } else {
            *reinterpret_cast<float2 *>(r + lane * NS + j) = make_float2(pe, ps);
          }
        }
        if constexpr (MODE == 3) put_post(t, pl, pb);
        else if (lane == 0) *reinterpret_cast<float *>(r + SRD - 2) = post(Acs + eb + cs);
        double x = C[0] + em(0);
        const double xl = from_next_lane(x, NINF);
        if constexpr (OPT) {
          double x1 = NL > 1 ? C[NL > 1 ? 1 : 0] + em(NL > 1 ? 1 : 0) : xl;
          const double xl2 = from_next_lane(x1, NINF);
          cs = wl_lse(cs + eb, x, ((skip >> 1) & 1u) ? x1 : NINF);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double x2 = j + 2 < NL ? C[j + 2 < NL ? j + 2 : 0] + em(j + 2 < NL ? j + 2 : 0) : j + 2 == NL ? xl : xl2;
            C[j] = wl_lse(C[j] + (((wild >> j) & 1u) ? ewj(j) : eb), x1, ((skip >> (j + 2)) & 1u) ? x2 : NINF);
            x1 = x2;
          }
        } else {
          cs = wl_lse(cs + eb, x);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double xn = j + 1 < NL ? C[j + 1 < NL ? j + 1 : 0] + em(j + 1 < NL ? j + 1 : 0) : xl;
            C[j] = wl_lse(C[j] + (((wild >> j) & 1u) ? ewj(j) : eb), xn);
            x = xn;
          }
        }
      }
    }
  };

  const int nb = (Tb + F - 1) / F;
  if (wave > 0 && nb > 0) produce(0);
  if constexpr (BACK && PF) {
    if (wave == 0 && Tb > 0) load_row(Tb - 1, An, Acsn);
  }
  __syncthreads();
  for (int kb = 0; kb < nb; ++kb) {
    if (wave == 0) {
      if constexpr (BACK) consume_back(kb);
      else consume(kb);
    } else if (kb + 1 < nb) {
      produce(kb + 1);
    }
    __syncthreads();
  }

  // ---- the end state ----
  if (!BACK && wave == 0) {
    const int i = L - 1, jj = i & (NL - 1);
    double cv = C[0], ov = O[0];
#pragma unroll
    for (int j = 1; j < NL; ++j)
      if (j == jj) { cv = C[j]; ov = O[j]; }
    double v = cs;
    if (L > 0) v = KIND == 0 ? wl_lse(ov, cv) : cv;
    if constexpr (OPT) {  // the last position may be empty: the states before it end the utterance too (every lane takes part)
      if (last_opt) {
        const int i2 = L >= 2 ? L - 2 : 0, j2 = i2 & (NL - 1);
        double c2 = C[0], o2 = O[0];
#pragma unroll
        for (int j = 1; j < NL; ++j)
          if (j == j2) { c2 = C[j]; o2 = O[j]; }
        c2 = __shfl(c2, i2 / NL);
        o2 = __shfl(o2, i2 / NL);
        const double v2 = L == 1 ? cs : KIND == 0 ? wl_lse(o2, c2) : c2;
        v = wl_lse(v, v2);
      }
    }
    if (too_long) v = NINF;
    if (lane == (L > 0 ? i / NL : 0)) {
      loss[b] = (float)(0.0 - v * LN2_D);  // (-inf: +inf; an empty utterance: +0)
      if (MODE == 1) ws.logp[b] = v;
    }
  }
}

// ---- the gradient's row stage: one wavefront per row (b, t), four per workgroup ----
constexpr int WLG_WAVES = 4;
constexpr int WLG_CH = 1024;  // columns per pass
constexpr int WLG_FIX = 40;   // fixed point: a posterior (in [0, 1]) in units of 2^-40, so |bin| < U 2^40

template <int KIND, bool OPT>
__global__ __launch_bounds__(64 * WLG_WAVES) void wild_grad_row_kernel(const Problem p, const int UP, const float *__restrict__ d_loss,
                                                                       const WlWs ws, void *__restrict__ grad) {
  constexpr int SLOT = KIND == 0 ? 16 : 8;  // bytes of a label position in a saved row; its first 8 are the two posteriors
  __shared__ unsigned long long bins_all[WLG_WAVES][WLG_CH];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long row = (long)blockIdx.x * WLG_WAVES + wv;
  if (row >= (long)p.B * p.T) return;  // (wavefront-uniform; nothing below synchronises beyond the wavefront)
  unsigned long long *const bins = bins_all[wv];
  const int b = (int)(row / p.T), t = (int)(row % p.T);
  const int V = p.V, blank = p.blank, xdt = p.xdtype, gdt = p.gdtype;
  const int Tb = frame_count(p, b);
  const int xesz = xdt == 0 ? 4 : 2, gesz = gdt == 0 ? 4 : 2;
  const char *const x = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb + (long)t * p.xst) * xesz;
  char *const g = reinterpret_cast<char *>(grad) + (size_t)((long)b * p.gsb + (long)t * p.gst) * gesz;
  const bool xvec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (xdt == 0 ? 15 : 7)) == 0;
  const bool gvec = ((V | p.gsb | p.gst) & 3) == 0 && (reinterpret_cast<uintptr_t>(grad) & (gdt == 0 ? 15 : 7)) == 0;

  // four consecutive elements of the gradient row from column k (k + 3 < V on the vector path; both paths convert alike)
  auto gput4 = [&](int k, const float4 r) {
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
  };

  // an infinite loss contributes nothing and its d_loss is not interpreted
  const double lp = ws.logp[b];
  const bool feasible = lp > -__builtin_inf() && lp < __builtin_inf();
  if (!(t < Tb) || !feasible) {  // a padded frame, an infeasible utterance: exactly zero
    for (int k = lane * 4; k < V; k += 256) gput4(k, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  const float dl = d_loss ? d_loss[b] : 1.f;
  if constexpr (OPT) {  // a weight of zero: +0 throughout, as above (0 * a negative element would be -0)
    if (dl == 0.f) {
      for (int k = lane * 4; k < V; k += 256) gput4(k, make_float4(0.f, 0.f, 0.f, 0.f));
      return;
    }
  }
  const float4 sv = *reinterpret_cast<const float4 *>(ws.stat + ((size_t)b * p.T + t) * 4);
  const float mx = sv.y, l2s = sv.z;
  const int L = label_count(p, b);  // (feasible: L <= U <= UP)
  const char *const r = reinterpret_cast<const char *>(ws.rows) + ((size_t)b * p.T + t) * ((size_t)wl_row_doubles(KIND, UP) * 8);
  const int32_t *const lab = label_row(p, b);

  float blk = 0.f, gam = 0.f;  // the blank's share and Gamma_t, lane-wise partial sums in a fixed order
  for (int c0 = 0; c0 < V; c0 += WLG_CH) {
#pragma unroll
    for (int q = 0; q < WLG_CH / 64; ++q) bins[lane + 64 * q] = 0ull;
    wave_lds_fence();
    for (int i = lane; i < L; i += 64) {
      const float2 pq = *reinterpret_cast<const float2 *>(r + (size_t)i * SLOT);
      const int tok = label_at(p, lab, i);
      const bool w = tok == WILD_LOSS_WILDCARD || (OPT && tok == WILD_LOSS_OPTIONAL);  // (OPT: a feasible utterance has no bad pair)
      const unsigned rel = (unsigned)(tok - c0);
      if (!w && emits(p, tok) && rel < (unsigned)WLG_CH)
        atomicAdd(&bins[rel], (unsigned long long)__float2ll_rn(__builtin_ldexpf(pq.x, WLG_FIX)));
      if (c0 == 0) {
        if (w) gam += pq.x;
        if (KIND == 1 && w) gam += pq.y;
        else blk += pq.y;
      }
    }
    if (c0 == 0) {
      if (lane == 0) blk += *reinterpret_cast<const float *>(r + (size_t)UP * SLOT);
      blk = wave_sum(blk);
      gam = wave_sum(gam);
    }
    wave_lds_fence();
    // logits: (1 - Gamma) softmax - gamma;  log-probabilities: -Gamma exp(x - LSE) - gamma
    const float c = p.wrt == 0 ? 1.f - gam : -gam;
#pragma unroll
    for (int q = 0; q < WLG_CH / 256; ++q) {
      const int k = c0 + lane * 4 + 256 * q;
      if (k < V) {
        const float4 xv = xvec ? wl_row_load4(x, k, xdt) : wl_row_load4_elem(x, k, V, xdt);
        float o[4];
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          const float bin = __builtin_ldexpf(__ll2float_rn((long long)bins[k - c0 + cc]), -WLG_FIX) + (k + cc == blank ? blk : 0.f);
          const float sm = c == 0.f ? 0.f : c * fexp2((xs[cc] - mx) * LOG2E - l2s);
          o[cc] = dl * (sm - bin);
        }
        gput4(k, make_float4(o[0], o[1], o[2], o[3]));
      }
    }
    wave_lds_fence();
  }
}

// ---- duration and expected_frame of ctc_amd_label_posterior: one workgroup per utterance and 64 label positions ----
// A lane is a position (a frame's 64 posteriors are one 256-byte read), a wavefront one of LS_SLICES contiguous runs of frames; the
// float64 partial sums meet in LDS and are added in the order of the frames: a fixed order, the same bits on every run.
constexpr int LS_SLICES = 8;

__global__ __launch_bounds__(64 * LS_SLICES) void label_stat_kernel(const Problem p, const double *__restrict__ logp,
                                                                    const float *__restrict__ post, float *__restrict__ duration,
                                                                    float *__restrict__ expected_frame) {
  __shared__ double sd[LS_SLICES][64], sm[LS_SLICES][64];
  const int b = blockIdx.x, lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int i = blockIdx.y * 64 + lane;
  const double lp = logp[b];
  const bool feasible = lp > -__builtin_inf() && lp < __builtin_inf();  // (then label_length <= U)
  const int Tb = frame_count(p, b);
  const int per = (Tb + LS_SLICES - 1) / LS_SLICES;
  const int t0 = sl * per, t1 = t0 + per < Tb ? t0 + per : Tb;
  double d = 0.0, m = 0.0;
  if (feasible && i < p.U && i < label_count(p, b)) {
    const float *const r = post + (size_t)b * p.T * p.U + i;
#pragma unroll 8
    for (int t = t0; t < t1; ++t) {
      const double v = (double)r[(size_t)t * p.U];
      d += v;
      m += (double)t * v;
    }
  }
  sd[sl][lane] = d;
  sm[sl][lane] = m;
  __syncthreads();
  if (sl != 0 || i >= p.U) return;
  d = 0.0; m = 0.0;
#pragma unroll
  for (int q = 0; q < LS_SLICES; ++q) { d += sd[q][lane]; m += sm[q][lane]; }
  duration[(size_t)b * p.U + i] = (float)d;
  expected_frame[(size_t)b * p.U + i] = d > 0.0 ? (float)(m / d) : -1.f;
}

template <int KIND, int NL, int MODE, bool WIN, bool OPT>
hipError_t launch_wild_loss(const Problem &p, double w2, float *loss, const WlArg<MODE> &ws, const int32_t *win, int wstride, hipStream_t st) {
  hipLaunchKernelGGL((wild_loss_kernel<KIND, NL, MODE, WIN, OPT>), dim3(p.B), dim3(WL_THREADS), 0, st, p, w2, loss, ws, win, wstride);
  return hipGetLastError();
}

// the window of a call: nullptr runs the WIN = false kernels; optional: the OPT kernels (never with a window)
struct WlWindow {
  const int32_t *ptr;
  int stride;
  bool optional;
};

#define CTC_WILD_LOSS_ROW(KIND, WIN, OPT)                                                                                             \
  {launch_wild_loss<KIND, 1, MODE, WIN, OPT>, launch_wild_loss<KIND, 2, MODE, WIN, OPT>, launch_wild_loss<KIND, 4, MODE, WIN, OPT>, \
   launch_wild_loss<KIND, 8, MODE, WIN, OPT>, launch_wild_loss<KIND, 16, MODE, WIN, OPT>}

template <int MODE>
hipError_t run_wild_mode(const Problem &p, double w2, float *loss, const WlArg<MODE> &ws, const WlWindow &fw, hipStream_t st) {
  typedef hipError_t Launch(const Problem &, double, float *, const WlArg<MODE> &, const int32_t *, int, hipStream_t);
  static Launch *const table[3][2][5] = {{CTC_WILD_LOSS_ROW(0, false, false), CTC_WILD_LOSS_ROW(1, false, false)},
                                         {CTC_WILD_LOSS_ROW(0, true, false), CTC_WILD_LOSS_ROW(1, true, false)},
                                         {CTC_WILD_LOSS_ROW(0, false, true), CTC_WILD_LOSS_ROW(1, false, true)}};
  const int NL = nl_for(p.U);
  const int lg = NL == 1 ? 0 : NL == 2 ? 1 : NL == 4 ? 2 : NL == 8 ? 3 : NL == 16 ? 4 : -1;
  if (lg < 0 || p.kind < 0 || p.kind > 1 || (fw.ptr && fw.optional)) return hipErrorInvalidValue;
  return table[fw.optional ? 2 : fw.ptr ? 1 : 0][p.kind][lg](p, w2, loss, ws, fw.ptr, fw.stride, st);
}

inline size_t wl_al(size_t x) { return (x + 255) & ~size_t(255); }

// the three regions of a workspace of wild_loss_workspace_bytes(want_grad = true)
WlWs wl_regions(const Problem &p, char *wsp) {
  const size_t rows = wl_al((size_t)p.B * p.T * wl_row_doubles(p.kind, 64 * nl_for(p.U)) * 8);
  return WlWs{reinterpret_cast<double *>(wsp), reinterpret_cast<float *>(wsp + rows),
              reinterpret_cast<double *>(wsp + rows + wl_al((size_t)p.B * p.T * 16))};
}

}  // namespace

// saved rows, then the row statistics, then log2 Z: each region rounded up to 256 bytes (include/ctc_amd.h has the formula)
size_t wild_loss_workspace_bytes(int kind, int B, int T, int U, bool want_grad) {
  if (!want_grad) return 0;
  const size_t rows = (size_t)B * T * wl_row_doubles(kind, 64 * nl_for(U)) * 8;
  return wl_al(rows) + wl_al((size_t)B * T * 16) + wl_al((size_t)B * 8);
}

hipError_t run_wild_loss(const Problem &p, float wildcard_log_weight, const float *d_loss, float *loss, void *grad, char *wsp,
                         hipStream_t st, const int32_t *frame_window, int window_stride, bool optional_wildcards) {
  const double w2 = (double)wildcard_log_weight * LOG2E_D;
  const WlWindow fw{frame_window, window_stride, optional_wildcards};
  if (!grad) return run_wild_mode<0>(p, w2, loss, WlWs{nullptr, nullptr, nullptr}, fw, st);
  const int UP = 64 * nl_for(p.U);
  const WlWs ws = wl_regions(p, wsp);
  if (hipError_t e = run_wild_mode<1>(p, w2, loss, ws, fw, st)) return e;
  if (p.T == 0) return hipSuccess;  // no rows
  if (hipError_t e = run_wild_mode<2>(p, w2, loss, ws, fw, st)) return e;
  const unsigned blocks = (unsigned)(((long)p.B * p.T + WLG_WAVES - 1) / WLG_WAVES);
  const dim3 grid(blocks), block(64 * WLG_WAVES);
  if (optional_wildcards) {
    if (p.kind == 0) hipLaunchKernelGGL((wild_grad_row_kernel<0, true>), grid, block, 0, st, p, UP, d_loss, ws, grad);
    else hipLaunchKernelGGL((wild_grad_row_kernel<1, true>), grid, block, 0, st, p, UP, d_loss, ws, grad);
  } else if (p.kind == 0) {
    hipLaunchKernelGGL((wild_grad_row_kernel<0, false>), grid, block, 0, st, p, UP, d_loss, ws, grad);
  } else {
    hipLaunchKernelGGL((wild_grad_row_kernel<1, false>), grid, block, 0, st, p, UP, d_loss, ws, grad);
  }
  return hipGetLastError();
}

hipError_t run_label_posterior(const Problem &p, float wildcard_log_weight, float *loss, float *label_posterior, float *blank_posterior,
                               float *duration, float *expected_frame, char *wsp, hipStream_t st, const int32_t *frame_window,
                               int window_stride, bool optional_wildcards) {
  const double w2 = (double)wildcard_log_weight * LOG2E_D;
  const WlWindow fw{frame_window, window_stride, optional_wildcards};
  WlPostWs ws;
  static_cast<WlWs &>(ws) = wl_regions(p, wsp);
  ws.post = label_posterior;
  ws.blk = blank_posterior;
  if (hipError_t e = run_wild_mode<1>(p, w2, loss, ws, fw, st)) return e;
  if (p.T > 0)
    if (hipError_t e = run_wild_mode<3>(p, w2, loss, ws, fw, st)) return e;
  if (duration && p.U > 0) {
    hipLaunchKernelGGL(label_stat_kernel, dim3(p.B, (p.U + 63) / 64), dim3(64 * LS_SLICES), 0, st, p, ws.logp, label_posterior, duration, expected_frame);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace ctc
