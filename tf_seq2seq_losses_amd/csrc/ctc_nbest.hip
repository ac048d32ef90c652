// N-best rescoring: the exact CTC loss of N label sequences per utterance: ctc_amd_nbest_loss (include/ctc_amd.h), DESIGN.md section 5.10.
//
// One workgroup per utterance and group of NBEST_G = 8 hypotheses, twelve wavefronts:
//   waves 0..7   the chains: wave g runs the alpha recursion of hypothesis n = blockIdx.y * 8 + g, NL label positions per lane
//                (position i = lane * NL + j), neighbour exchange with DPP (from_prev_lane), state in registers;
//   waves 8..11  producers: stream the frame's row ONCE (float32 / bfloat16 / float16, run-time switch) for its max and sum, and
//                gather x[t, label[n][i]] of all eight hypotheses from that row (in flight or L2-resident then) into an LDS ring
//                one block of frames ahead of the chains.  Every producer thread keeps the 2 NL labels it gathers in registers.
//                No V-wide row is staged in LDS: any V costs no LDS.
// Numerics: log domain.  The state is the float64 base-2 logarithm of the forward mass; a log-sum-exp is the float64 maximum plus a
// float32 v_log_f32 of a sum of float32 v_exp_f32 of float64 DIFFERENCES (ctc_common.h lse2(double, double), here for two and three
// operands and with a true -inf as log(0): nothing is rescaled, nothing can be flushed, an impossible state stays -inf exactly).
// The emission of a frame enters as ((double)x - (double)max) * log2(e) - log2(sum): the subtraction is exact in float64, so a
// row of 1e10 costs nothing, and the float32 row statistics are the only float32 quantities that are not differences.
//
// States as in ctc_align.hip.  Classic: O[i] = the last frame emitted label i (open), C[i] = labels 0..i are done and the last
// frame was blank (closed), plus the start state `cs` (blank so far) that lane 0 feeds into position 0.  Simplified: S[i].
//   O'[i] = lse(O[i], C[i-1], O[i-1] if label[i] != label[i-1]) + e[label[i]]
//   C'[i] = lse(C[i], O[i]) + e[blank]
//   S'[i] = lse(S[i] + e[blank], S[i-1] + e[label[i]])
// The result of hypothesis (b, n) is a function of its own labels and of the ring rows of utterance b, which are the same bits
// for every group, position and N: no hypothesis can see another.
//
// The gradient of sum_n weight[b, n] * loss[b, n] (ctc_amd_nbest_loss_grad) runs the same kernel body three
// times over (template parameter MODE) and one row kernel behind it:
//   MODE 0  the loss alone, as above;
//   MODE 1  the same alpha sweep, bit for bit, that also stores every chain's state of every frame (float64) and the final log2 P,
//           and the producers' row statistics, to the workspace;
//   MODE 2  the beta sweep: same grid and roles, frames from T_b - 1 down (the producers gather in reverse order).  Per frame a
//           chain reads its own saved row, forms the posteriors 2^(alpha + beta - log2 P) in float64 and writes them as float32
//           pairs over the slots it has just read (only the chain's own lane touches a slot), then steps beta back over the frame;
//   MODE 3  the alpha sweep of MODE 1 that stores one state per BLOCK of frames (before its first frame) instead of one per frame:
//           the first launch of ctc_amd_nbest_loss_grad_ckpt (nbest_ckpt_bwd_kernel below is the second);
//   nbest_grad_row_kernel  one wavefront per row (b, t): adds weight * posterior of every label position of every feasible
//           hypothesis into 64-bit fixed-point LDS bins by token (integer atomics: no arrival order in the sum), the vocabulary
//           in passes of 1024 columns, and streams the row out: softmax from the saved statistics times the weight sum, minus bins.
// A saved row of hypothesis (b, n) and frame t: per label position i the pair (O, C) (classic, AFTER frame t) or S (simplified,
// BEFORE frame t), then the start state; (2 or 1) * UP + 2 doubles.  After the beta sweep the first 8 bytes of position i hold
//   classic:    (posterior of O[i] after frame t = frame t emits label i,   posterior of C[i] = a blank behind label i)
//   simplified: (alpha_{t-1}[i-1] e_t[label i] beta_t[i] / P,               alpha_{t-1}[i] e_t[blank] beta_t[i] / P)
// and the start state's slot its blank posterior: .x goes to the token's column, .y to the blank's, on both lattices.
#include "ctc_common.h"
#include "ctc_lane_ops.h"
#include "ctc_launch.h"

namespace ctc {
namespace {

constexpr int NBEST_PW = 4;                                  // producer wavefronts
constexpr int NBEST_PT = 64 * NBEST_PW;                      // producer threads
constexpr int NBEST_THREADS = 64 * NBEST_G + NBEST_PT;       // 768
constexpr int NBEST_RING = 1024;                             // label emissions per hypothesis and ring buffer: frames per block = 1024 / UP
constexpr double LOG2E_D = 1.44269504088896340736;

__device__ __forceinline__ float4 nb_row_load4(const char *row, int k, int dt) {
  if (dt == 0) return *reinterpret_cast<const float4 *>(row + (size_t)k * 4);
  const uint2 u = *reinterpret_cast<const uint2 *>(row + (size_t)k * 2);
  return make_float4(h16_to_f32((unsigned short)(u.x & 0xffffu), dt), h16_to_f32((unsigned short)(u.x >> 16), dt),
                     h16_to_f32((unsigned short)(u.y & 0xffffu), dt), h16_to_f32((unsigned short)(u.y >> 16), dt));
}
// the same four elements one by one (unaligned rows, V no multiple of 4): -inf past the row, which adds nothing to either statistic
__device__ __forceinline__ float4 nb_row_load4_elem(const char *row, int k, int V, int dt) {
  const float ninf = -__builtin_inff();
  return make_float4(row_load1(row, k, dt), k + 1 < V ? row_load1(row, k + 1, dt) : ninf, k + 2 < V ? row_load1(row, k + 2, dt) : ninf,
                     k + 3 < V ? row_load1(row, k + 3, dt) : ninf);
}
// running (max, sum of exp(x - max)) of one lane: four more elements (both access paths end here: identical bits)
__device__ __forceinline__ void nb_stat_add4(float &m, float &s, const float4 v) {
  const float mn = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
  s = s * fexp2((m - mn) * LOG2E) +
      ((fexp2((v.x - mn) * LOG2E) + fexp2((v.y - mn) * LOG2E)) + (fexp2((v.z - mn) * LOG2E) + fexp2((v.w - mn) * LOG2E)));
  m = mn;
}

// base-2 log(2^a + 2^b [+ 2^c]) of float64 operands that may be -inf (log 0): differences against the maximum, or against 0
// when every operand is -inf (then every term is exp2(-inf) = 0 and the result log2(0) = -inf, without a NaN on the way)
__device__ __forceinline__ double nb_lse(double a, double b) {
  const double m = fmax(a, b);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2(fexp2((float)(a - mm)) + fexp2((float)(b - mm)));
}
__device__ __forceinline__ double nb_lse(double a, double b, double c) {
  const double m = fmax(fmax(a, b), c);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2((fexp2((float)(a - mm)) + fexp2((float)(b - mm))) + fexp2((float)(c - mm)));
}

// the token of label position i of hypothesis row `row` with L labels, -1 where nothing can be emitted
__device__ __forceinline__ int nb_token(const Problem &p, long row, int L, int i) {
  if (i < 0 || i >= L) return -1;
  const int tok = label_at(p, p.labels + row * p.label_stride, i);
  return emits(p, tok) ? tok : -1;
}

// the gradient's workspace (MODE 0: unused)
struct NbWs {
  double *rows;  // [B * N][T][SRD] saved alpha rows, then the posteriors
  float *stat;   // [B][T][4] x[blank], row max, log2 sum exp(x - max) of every frame
  double *logp;  // [B * N] log2 P, -inf for an infeasible hypothesis
};
constexpr int nb_row_doubles(int kind, int UP) { return (kind == 0 ? 2 : 1) * UP + 2; }

template <int KIND, int NL, int MODE>
__global__ __launch_bounds__(NBEST_THREADS) void nbest_kernel(const Problem p, const int N, float *__restrict__ loss, const NbWs ws) {
  constexpr int UP = 64 * NL;
  constexpr int NS = (KIND == 0 ? 2 : 1) * NL;        // doubles of a saved row per lane
  constexpr int SRD = nb_row_doubles(KIND, UP);
  constexpr bool PF = NL <= 4;                        // MODE 2: the next frame's saved row is requested one frame ahead
  constexpr int F = NBEST_RING / UP;                  // frames per ring buffer: 16, 8, 4, 2, 1
  constexpr int FR = NBEST_G * UP;                    // ring floats per frame: the eight hypotheses' emissions
  constexpr int CNT = FR / NBEST_PT;                  // gathers per producer thread and frame: 2 NL
  constexpr int FPW = F / NBEST_PW > 0 ? F / NBEST_PW : 1;  // frames per producer wavefront and block, all in flight together
  const double NINF = -__builtin_inf();

  __shared__ __attribute__((aligned(16))) float ring[2 * F * FR];  // [buffer][frame][hypothesis][position]
  __shared__ __attribute__((aligned(16))) float stat[2 * F * 4];   // [buffer][frame]: x[blank], row max, log2 sum exp(x - max)

  const int b = blockIdx.x, n0 = blockIdx.y * NBEST_G;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool chain = wave < NBEST_G;
  const int V = p.V, blank = p.blank, dt = p.xdtype;
  const int Tb = frame_count(p, b);
  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  // vector row accesses (16 bytes of float32, 8 bytes of 16-bit elements) need aligned rows; element-wise otherwise
  const bool vec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (dt == 0 ? 15 : 7)) == 0;

  // label count of hypothesis n of this utterance: 0 when there is none or it has too many labels (reported +inf at the end)
  auto count_of = [&](int n, bool &too_long) {
    too_long = false;
    if (n >= N) return 0;
    const int L = label_count(p, b * N + n);
    too_long = too_many_labels(p, L);
    return too_long ? 0 : L;
  };

  const int nb = (Tb + F - 1) / F;
  // The two roles run their own loops (the branch is wavefront-uniform) and meet at one raw barrier per block of frames: the
  // chains' state is then not live in the producers' code, nor the producers' gather offsets in the chains'.
  if (chain) {
    // ---- the chains (waves 0..7) ----
    const int n = n0 + wave;
    const long hrow = (long)b * N + n;
    bool too_long = false;
    const int L = count_of(n, too_long);
    double O[NL], C[NL];  // simplified: C is S, O unused
    unsigned allow = 0;   // classic: bit j = label[i] differs from label[i-1]
    double cs = 0.0;      // the start state: blank so far
#pragma unroll
    for (int j = 0; j < NL; ++j) { O[j] = NINF; C[j] = NINF; }
    if (KIND == 0) {
      int prev = nb_token(p, hrow, L, lane * NL - 1);
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const int i = lane * NL + j;
        const int tok = nb_token(p, hrow, L, i);
        if (i > 0 && tok != prev) allow |= 1u << j;
        prev = tok;
      }
    }
    // (n >= N: never dereferenced.)  MODE 3: one row per block of F frames, the state BEFORE the block's first frame
    double *const myrows = MODE == 3 ? ws.rows + (size_t)hrow * ((p.T + F - 1) / F) * SRD
                           : MODE != 0 ? ws.rows + (size_t)hrow * p.T * SRD : nullptr;
    // MODE 2: O / C / cs hold beta, the mass of the frames still to come; behind the last frame only the end states have any
    double lP = 0.0;
    bool active = n < N;
    int allow_nx = 0;  // classic: the `allow` bit of the next lane's first position
    if constexpr (MODE == 2) {
      if (active) lP = ws.logp[hrow];
      active = active && lP > NINF && lP < -NINF;
#pragma unroll
      for (int j = 0; j < NL; ++j) O[j] = C[j] = (lane * NL + j == L - 1) ? 0.0 : NINF;
      cs = L == 0 ? 0.0 : NINF;
      if (KIND == 0) allow_nx = fused::from_next_lane_i((int)(allow & 1u), 0);
    }
    auto load_row = [&](int t, double (&A)[NS], double &Acs) {
      const double *const r = myrows + (size_t)t * SRD;
#pragma unroll
      for (int q = 0; q < NS; ++q) A[q] = r[lane * NS + q];
      Acs = r[SRD - 2];
    };

    auto consume = [&](int kb) {
      const int t0 = kb * F;
      const int nf = Tb - t0 < F ? Tb - t0 : F;
      const float *const rb = ring + (kb & 1) * F * FR + wave * UP + lane * NL;
      const float *const sb = stat + (kb & 1) * F * 4;
      if constexpr (MODE == 3) {  // the block's checkpoint, in the layout of a MODE 1 row
        double *const r = myrows + (size_t)kb * SRD;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          if (KIND == 0) *reinterpret_cast<double2 *>(r + lane * NS + 2 * j) = make_double2(O[j], C[j]);
          else r[lane * NS + j] = C[j];
        }
        if (lane == 0) r[SRD - 2] = cs;
      }
      for (int f = 0; f < nf; ++f) {
        float e[NL];
        fused::ld_slots<NL>(rb + f * FR, e);
        const float4 sv = *reinterpret_cast<const float4 *>(sb + f * 4);
        const double Md = (double)sv.y, nl2s = -(double)sv.z;
        const double eb = fma((double)sv.x - Md, LOG2E_D, nl2s);
        // (the emission of position j in the lattice's units, made where it is used: no float64 copy of the row stays live)
        auto em = [&](int j) { return fma((double)e[j] - Md, LOG2E_D, nl2s); };
        double *const r = MODE == 1 ? myrows + (size_t)(t0 + f) * SRD : nullptr;
        if (MODE == 1 && KIND == 1) {  // the state BEFORE the frame
#pragma unroll
          for (int j = 0; j < NL; ++j) r[lane * NS + j] = C[j];
          if (lane == 0) r[SRD - 2] = cs;
        }
        if (KIND == 0) {
          const double pO = from_prev_lane(O[NL - 1], NINF);
          const double pC = from_prev_lane(C[NL - 1], cs);
#pragma unroll
          for (int j = NL - 1; j >= 0; --j) {
            const double qO = j > 0 ? O[j > 0 ? j - 1 : 0] : pO;
            const double qC = j > 0 ? C[j > 0 ? j - 1 : 0] : pC;
            const double a2 = ((allow >> j) & 1u) ? qO : NINF;
            const double o = nb_lse(O[j], qC, a2) + em(j);
            C[j] = nb_lse(C[j], O[j]) + eb;
            O[j] = o;
          }
        } else {
          const double pS = from_prev_lane(C[NL - 1], cs);
#pragma unroll
          for (int j = NL - 1; j >= 0; --j) {
            const double q = j > 0 ? C[j > 0 ? j - 1 : 0] : pS;
            C[j] = nb_lse(C[j] + eb, q + em(j));
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

    // MODE 2: block kb holds the frames T_b - 1 - kb F downwards
    double An[NS], Acsn = 0.0;
    auto consume_back = [&](int kb) {
      const int t0 = kb * F;
      const int nf = Tb - t0 < F ? Tb - t0 : F;
      const float *const rb = ring + (kb & 1) * F * FR + wave * UP + lane * NL;
      const float *const sb = stat + (kb & 1) * F * 4;
      for (int f = 0; f < nf; ++f) {
        const int t = Tb - 1 - (t0 + f);
        float e[NL];
        fused::ld_slots<NL>(rb + f * FR, e);
        const float4 sv = *reinterpret_cast<const float4 *>(sb + f * 4);
        const double Md = (double)sv.y, nl2s = -(double)sv.z;
        const double eb = fma((double)sv.x - Md, LOG2E_D, nl2s);
        auto em = [&](int j) { return fma((double)e[j] - Md, LOG2E_D, nl2s); };
        double A[NS], Acs;
        if constexpr (PF) {
#pragma unroll
          for (int q = 0; q < NS; ++q) A[q] = An[q];
          Acs = Acsn;
          if (t > 0) load_row(t - 1, An, Acsn);
        } else {
          load_row(t, A, Acs);
        }
        double *const r = myrows + (size_t)t * SRD;
        auto post = [&](double l2) { return fexp2((float)(l2 - lP)); };
        if (KIND == 0) {
#pragma unroll
          for (int j = 0; j < NL; ++j)
            *reinterpret_cast<float2 *>(r + lane * NS + 2 * j) = make_float2(post(A[2 * j] + O[j]), post(A[2 * j + 1] + C[j]));
          if (lane == 0) *reinterpret_cast<float *>(r + SRD - 2) = post(Acs + cs);
          // beta back over frame t: x = what entering O[i] with this frame is worth
          double x = O[0] + em(0);
          const double xl = from_next_lane(x, NINF);
          cs = nb_lse(cs + eb, x);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double xn = j + 1 < NL ? O[j + 1 < NL ? j + 1 : 0] + em(j + 1 < NL ? j + 1 : 0) : xl;
            const bool al = j + 1 < NL ? ((allow >> (j + 1)) & 1u) != 0 : allow_nx != 0;
            const double cb = C[j] + eb;
            O[j] = nb_lse(x, cb, al ? xn : NINF);
            C[j] = nb_lse(cb, xn);
            x = xn;
          }
        } else {
          const double ap0 = from_prev_lane(A[NL - 1], Acs);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double ap = j > 0 ? A[j > 0 ? j - 1 : 0] : ap0;
            *reinterpret_cast<float2 *>(r + lane * NS + j) = make_float2(post(ap + em(j) + C[j]), post(A[j] + eb + C[j]));
          }
          if (lane == 0) *reinterpret_cast<float *>(r + SRD - 2) = post(Acs + eb + cs);
          double x = C[0] + em(0);
          const double xl = from_next_lane(x, NINF);
          cs = nb_lse(cs + eb, x);
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double xn = j + 1 < NL ? C[j + 1 < NL ? j + 1 : 0] + em(j + 1 < NL ? j + 1 : 0) : xl;
            C[j] = nb_lse(C[j] + eb, xn);
            x = xn;
          }
        }
      }
    };

    fused::block_barrier();
    if constexpr (MODE == 2 && PF) {
      if (active && Tb > 0) load_row(Tb - 1, An, Acsn);
    }
    for (int kb = 0; kb < nb; ++kb) {
      if constexpr (MODE == 2) {
        if (active) consume_back(kb);
      } else {
        if (n < N) consume(kb);
      }
      fused::block_barrier();
    }

    // the end state
    if (MODE != 2 && n < N) {
      const int i = L - 1, jj = i & (NL - 1);
      double cv = C[0], ov = O[0];
#pragma unroll
      for (int j = 1; j < NL; ++j)
        if (j == jj) { cv = C[j]; ov = O[j]; }
      double v = cs;
      if (L > 0) v = KIND == 0 ? nb_lse(ov, cv) : cv;
      if (too_long) v = NINF;
      if (lane == (L > 0 ? i / NL : 0)) {
        loss[hrow] = (float)(0.0 - v * LN2_D);  // (-inf: +inf; an empty utterance: +0)
        if (MODE == 1 || MODE == 3) ws.logp[hrow] = v;
      }
    }
  } else {
    // ---- the producers (waves 8..11): the labels a thread gathers are the same every frame ----
    const int tp = tid - 64 * NBEST_G, pw = wave - NBEST_G;
    unsigned goff[CNT];   // byte offset of the label's element in a row (the blank's where nothing can be emitted: a valid address)
    unsigned gvalid = 0;  // bit c: gather c is an emission
#pragma unroll
    for (int c = 0; c < CNT; ++c) {
      const int idx = tp + NBEST_PT * c, g = idx / UP, i = idx % UP;
      bool tl;
      const int Lg = count_of(n0 + g, tl);
      const int tok = nb_token(p, (long)b * N + n0 + g, Lg, i);
      goff[c] = (unsigned)(tok >= 0 ? tok : blank) * (unsigned)esz;
      if (tok >= 0) gvalid |= 1u << c;
    }
    // the frame a block's position stands for (MODE 2 runs backwards); past the utterance's end its last, valid memory whose
    // results are never stored
    auto real_t = [&](int t) {
      const int c = t < Tb ? t : Tb - 1;
      return MODE == 2 ? Tb - 1 - c : c;
    };
    auto frame_row = [&](int t) { return xb + (size_t)((long)real_t(t) * p.xst) * esz; };

    auto produce = [&](int kb) {
      const int t0 = kb * F;
      float *const rb = ring + (kb & 1) * F * FR;
      float *const sb = stat + (kb & 1) * F * 4;
      // the gathers of the block: F * CNT = 32 per thread, in two batches of 16 loads in flight together, stored as they arrive
      constexpr int BATCH = 16;
#pragma unroll
      for (int k0 = 0; k0 < F * CNT; k0 += BATCH) {
        float e[BATCH];
        if (dt == 0) {
#pragma unroll
          for (int k = 0; k < BATCH; ++k) {
            const int f = (k0 + k) / CNT, c = (k0 + k) % CNT;
            e[k] = *reinterpret_cast<const float *>(frame_row(t0 + f) + goff[c]);
          }
        } else {
          unsigned short h[BATCH];
#pragma unroll
          for (int k = 0; k < BATCH; ++k) {
            const int f = (k0 + k) / CNT, c = (k0 + k) % CNT;
            h[k] = *reinterpret_cast<const unsigned short *>(frame_row(t0 + f) + goff[c]);
          }
#pragma unroll
          for (int k = 0; k < BATCH; ++k) e[k] = h16_to_f32(h[k], dt);
        }
#pragma unroll
        for (int k = 0; k < BATCH; ++k)
          if (!((gvalid >> ((k0 + k) % CNT)) & 1u)) e[k] = -__builtin_inff();
#pragma unroll
        for (int k = 0; k < BATCH; ++k) {
          const int f = (k0 + k) / CNT, c = (k0 + k) % CNT;
          if (t0 + f < Tb) rb[f * FR + tp + NBEST_PT * c] = e[k];
        }
      }
      // row statistics: this wavefront's frames f = pw + 4 q
      const char *row[FPW];
      float m[FPW], s[FPW], ebl[FPW];
#pragma unroll
      for (int q = 0; q < FPW; ++q) {
        const int f = pw + NBEST_PW * q;
        const int t = real_t(f < F ? t0 + f : Tb);
        row[q] = xb + (size_t)((long)t * p.xst) * esz;
        ebl[q] = row_load1(row[q], blank, dt);
        m[q] = -3.402823466e38f; s[q] = 0.f;
      }
      if (p.wrt == 0) {
        for (int k = lane * 4; k < V; k += 256) {
          float4 v[FPW];
#pragma unroll
          for (int q = 0; q < FPW; ++q) v[q] = vec ? nb_row_load4(row[q], k, dt) : nb_row_load4_elem(row[q], k, V, dt);
#pragma unroll
          for (int q = 0; q < FPW; ++q) nb_stat_add4(m[q], s[q], v[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < FPW; ++q) {
        const int f = pw + NBEST_PW * q;
        float M = 0.f, l2s = 0.f;
        if (p.wrt == 0) {
          M = wave_max(m[q]);
          const float S = wave_sum(s[q] * fexp2((m[q] - M) * LOG2E));
          l2s = flog2(S);
          if (!(S > 0.f)) { M = 0.f; l2s = __builtin_inff(); }  // a row of -inf: every emission of the frame is -inf
        }
        if (lane == 0 && f < F && t0 + f < Tb) {
          *reinterpret_cast<float4 *>(sb + f * 4) = make_float4(ebl[q], M, l2s, 0.f);
          if ((MODE == 1 || MODE == 3) && blockIdx.y == 0) *reinterpret_cast<float4 *>(ws.stat + ((size_t)b * p.T + t0 + f) * 4) = make_float4(ebl[q], M, l2s, 0.f);
        }
      }
    };

    if (nb > 0) produce(0);
    fused::block_barrier();
    for (int kb = 0; kb < nb; ++kb) {
      if (kb + 1 < nb) produce(kb + 1);
      fused::block_barrier();
    }
  }
}

// ---- the gradient's row stage: one wavefront per row (b, t), four per workgroup ----
constexpr int NBG_WAVES = 4;
constexpr int NBG_CH = 1024;     // columns per pass
constexpr int NBG_FIX = 40;      // fixed point: units of 2^(e - 40) with 2^e > max_n |weight[b, n]|, so |bin| < N 2^40

template <int KIND>
__global__ __launch_bounds__(64 * NBG_WAVES) void nbest_grad_row_kernel(const Problem p, const int N, const int UP,
                                                                        const float *__restrict__ weight, const NbWs ws,
                                                                        void *__restrict__ grad) {
  constexpr int SLOT = KIND == 0 ? 16 : 8;  // bytes of a label position in a saved row; its first 8 are (token, blank) posteriors
  __shared__ unsigned long long bins_all[NBG_WAVES][NBG_CH];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long row = (long)blockIdx.x * NBG_WAVES + wv;
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

  // the weights of the hypotheses that count (lane n: hypothesis n; N <= 64): an infinite loss contributes nothing and its weight
  // is not interpreted
  float wn = 0.f;
  if (lane < N && t < Tb) {
    const double lp = ws.logp[(long)b * N + lane];
    if (lp > -__builtin_inf() && lp < __builtin_inf()) wn = weight[(long)b * N + lane];
  }
  const float wsum = wave_sum(wn);
  const float wmax = wave_max(fabsf(wn));
  if (!(t < Tb) || !(wmax > 0.f)) {  // a padded frame, no feasible hypothesis (or zero weights alone): exactly zero
    for (int k = lane * 4; k < V; k += 256) gput4(k, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  const int fe = __builtin_amdgcn_frexp_expf(wmax);  // wmax = m 2^fe, m in [0.5, 1)
  const float4 sv = *reinterpret_cast<const float4 *>(ws.stat + ((size_t)b * p.T + t) * 4);
  const float mx = sv.y, l2s = sv.z;
  const bool wrt_logits = p.wrt == 0;
  constexpr int SRD_B = 8;  // bytes per double
  const size_t srd = (size_t)nb_row_doubles(KIND, UP) * SRD_B;

  float blk = 0.f;  // the blank's share, lane-wise partial sums in a fixed order
  for (int c0 = 0; c0 < V; c0 += NBG_CH) {
#pragma unroll
    for (int q = 0; q < NBG_CH / 64; ++q) bins[lane + 64 * q] = 0ull;
    wave_lds_fence();
    for (int n = 0; n < N; ++n) {
      const float w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wn), n));
      if (w == 0.f) continue;
      const long hrow = (long)b * N + n;
      const int L = label_count(p, (int)hrow);  // (feasible: L <= U <= UP)
      const char *const r = reinterpret_cast<const char *>(ws.rows) + ((size_t)hrow * p.T + t) * srd;
      const int32_t *const lab = p.labels + hrow * p.label_stride;
      for (int i = lane; i < L; i += 64) {
        const float2 pq = *reinterpret_cast<const float2 *>(r + (size_t)i * SLOT);
        const int tok = label_at(p, lab, i);
        const unsigned rel = (unsigned)(tok - c0);
        if (emits(p, tok) && rel < (unsigned)NBG_CH)
          atomicAdd(&bins[rel], (unsigned long long)__float2ll_rn(__builtin_ldexpf(w * pq.x, NBG_FIX - fe)));
        if (c0 == 0) blk += w * pq.y;
      }
      if (c0 == 0 && lane == 0) blk += w * *reinterpret_cast<const float *>(r + (size_t)UP * SLOT);
    }
    if (c0 == 0) blk = wave_sum(blk);
    wave_lds_fence();
#pragma unroll
    for (int q = 0; q < NBG_CH / 256; ++q) {
      const int k = c0 + lane * 4 + 256 * q;
      if (k < V) {
        float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (wrt_logits) xv = xvec ? nb_row_load4(x, k, xdt) : nb_row_load4_elem(x, k, V, xdt);
        float r[4];
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float bin = __builtin_ldexpf(__ll2float_rn((long long)bins[k - c0 + c]), fe - NBG_FIX) + (k + c == blank ? blk : 0.f);
          // WRT_LOGITS: sum_n w_n (softmax(x)[k] - gamma_n[k]);  WRT_LOGPROBS: - sum_n w_n gamma_n[k]
          r[c] = wrt_logits ? wsum * fexp2((xs[c] - mx) * LOG2E - l2s) - bin : -bin;
        }
        gput4(k, make_float4(r[0], r[1], r[2], r[3]));
      }
    }
    wave_lds_fence();
  }
}

// ---- the gradient from block checkpoints (ctc_amd_nbest_loss_grad_ckpt): the fused backward sweep ----
// Behind nbest_kernel MODE 3 (the alpha sweep of MODE 0 that stores every chain's state BEFORE each block of F frames, the row
// statistics and log2 P).  One workgroup per utterance, the twelve wavefronts and roles of nbest_kernel; the groups of eight
// hypotheses one after the other.  Blocks of frames are aligned to frame 0 and walked from the last (partial) one down, two raw
// barriers per block:
//   phase A  chains: load the block's checkpoint, re-run the alpha step over the ring block, keep the rows in registers (NS * F = 32
//                    or 16 doubles; the frame loops are unrolled, every row index is static), the start state's values in LDS;
//            producers: the row stage of the block the sweep handled just before -- wavefront pw takes frames pw, pw + 4, .. with
//                    bins of its own, the arithmetic of nbest_grad_row_kernel: weight * posterior into 64-bit fixed-point bins by
//                    token, then the row out: weight sum * softmax - bins;
//   phase B  chains: beta back over the same ring block; per frame the token posterior of every position goes to the LDS posterior
//                    block as one float32, the blank's share of the hypothesis as one wave-reduced float32;
//            producers: gather the next (earlier) block's emissions into the other ring buffer, its statistics from the workspace.
// Nothing per frame reaches memory.  More than one group: the first writes weight sum * softmax - bins to a float32 accumulator,
// later ones subtract their bins, the last converts to the gradient (the same thread owns an element in every group).
struct NbCk {
  const double *ck;    // [B * N][ceil(T / F)][SRD] the chains' state before every block, in the layout of a MODE 1 row
  const float *stat;   // [B][T][4]
  const double *logp;  // [B * N]
  float *acc;          // [B][T][V], N > NBEST_G only
};

// four consecutive elements of a gradient row from column k, in its element type; element-wise where the row is not aligned
__device__ __forceinline__ void nb_grad_put4(char *g, int k, int V, int gdt, bool gvec, const float4 r) {
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

template <int KIND, int NL>
__global__ __launch_bounds__(NBEST_THREADS) void nbest_ckpt_bwd_kernel(const Problem p, const int N, const float *__restrict__ weight,
                                                                       const NbCk ws, void *__restrict__ grad) {
  constexpr int UP = 64 * NL;
  constexpr int NS = (KIND == 0 ? 2 : 1) * NL;
  constexpr int SRD = nb_row_doubles(KIND, UP);
  constexpr int F = NBEST_RING / UP;          // 16, 8, 4
  constexpr int FR = NBEST_G * UP;
  constexpr int CNT = FR / NBEST_PT;          // 2 NL
  constexpr int FPW = F / NBEST_PW;           // frames per producer wavefront and block: 4, 2, 1
  static_assert(NL == 1 || NL == 2 || NL == 4, "register rows: U <= 256");
  const double NINF = -__builtin_inf();

  __shared__ __attribute__((aligned(16))) float ring[2 * F * FR];   // [buffer][frame][hypothesis][position]
  __shared__ __attribute__((aligned(16))) float stat[2 * F * 4];    // [buffer][frame]
  __shared__ __attribute__((aligned(16))) float pst[F * FR];        // [frame][hypothesis][position] token posteriors of one block
  __shared__ float bsh[F * NBEST_G];                                // [frame][hypothesis] the blank's share
  __shared__ double csb[NBEST_G * F];                               // [hypothesis][frame] alpha of the start state
  __shared__ int tokt[FR];                                          // [hypothesis][position] token, -1: no emission
  __shared__ unsigned long long bins_all[NBEST_PW][NBG_CH];

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool chain = wave < NBEST_G;
  const int V = p.V, blank = p.blank, dt = p.xdtype, gdt = p.gdtype;
  const int Tb = frame_count(p, b);
  const int esz = dt == 0 ? 4 : 2, gesz = gdt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  char *const gb = reinterpret_cast<char *>(grad) + (size_t)((long)b * p.gsb) * gesz;
  const bool xvec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (dt == 0 ? 15 : 7)) == 0;
  const bool gvec = ((V | p.gsb | p.gst) & 3) == 0 && (reinterpret_cast<uintptr_t>(grad) & (gdt == 0 ? 15 : 7)) == 0;
  const int nbk = (p.T + F - 1) / F;     // checkpoint rows per hypothesis
  const int ngrp = (N + NBEST_G - 1) / NBEST_G;

  // the weights that count, over ALL N hypotheses of the utterance (lane n: hypothesis n), every wavefront for itself: an infinite
  // loss contributes nothing and its weight is not interpreted
  float wn = 0.f;
  if (lane < N) {
    const double lp = ws.logp[(long)b * N + lane];
    if (lp > NINF && lp < -NINF) wn = weight[(long)b * N + lane];
  }
  const float wsum = wave_sum(wn);
  const float wmax = wave_max(fabsf(wn));
  // padded frames, and every frame without a feasible hypothesis (or with zero weights alone): exactly zero
  const int Tz = wmax > 0.f ? Tb : 0;
  for (int t = Tz + wave; t < p.T; t += NBEST_THREADS / 64) {
    char *const g = gb + (size_t)((long)t * p.gst) * gesz;
    for (int k = lane * 4; k < V; k += 256) nb_grad_put4(g, k, V, gdt, gvec, make_float4(0.f, 0.f, 0.f, 0.f));
  }
  if (Tz == 0) return;  // (the same verdict in every wavefront: nobody waits at a barrier)
  const int fe = __builtin_amdgcn_frexp_expf(wmax);
  const int nb = (Tb + F - 1) / F;

  auto count_of = [&](int n, bool &too_long) {
    too_long = false;
    if (n >= N) return 0;
    const int L = label_count(p, b * N + n);
    too_long = too_many_labels(p, L);
    return too_long ? 0 : L;
  };

  if (chain) {
    // ---- the chains (waves 0..7) ----
    for (int grp = 0; grp < ngrp; ++grp) {
      const int n = grp * NBEST_G + wave;
      const long hrow = (long)b * N + n;
      bool too_long = false;
      const int L = count_of(n, too_long);
      unsigned allow = 0;
      if (KIND == 0) {
        int prev = nb_token(p, hrow, L, lane * NL - 1);
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          const int i = lane * NL + j;
          const int tok = nb_token(p, hrow, L, i);
          if (i > 0 && tok != prev) allow |= 1u << j;
          prev = tok;
        }
      }
      const int allow_nx = KIND == 0 ? fused::from_next_lane_i((int)(allow & 1u), 0) : 0;
      double lP = 0.0;
      bool active = n < N;
      if (active) {
        lP = ws.logp[hrow];
        active = lP > NINF && lP < -NINF && weight[hrow] != 0.f;  // (a zero weight: the row stage skips the hypothesis as well)
      }
      // beta: the mass of the frames still to come; behind the last frame only the end states have any
      double O[NL], C[NL];  // simplified: C is S, O unused
#pragma unroll
      for (int j = 0; j < NL; ++j) O[j] = C[j] = (lane * NL + j == L - 1) ? 0.0 : NINF;
      double cs = L == 0 ? 0.0 : NINF;
      const double *const myck = ws.ck + (size_t)hrow * nbk * SRD;  // (n >= N: never dereferenced)
      auto post = [&](double l2) { return fexp2((float)(l2 - lP)); };

      fused::block_barrier();
      for (int kb = nb - 1; kb >= 0; --kb) {
        const int nf = Tb - kb * F < F ? Tb - kb * F : F;
        const float *const rb = ring + (kb & 1) * F * FR + wave * UP + lane * NL;
        const float *const sb = stat + (kb & 1) * F * 4;
        double RA[F][NS];  // alpha rows of the block: classic (O, C) AFTER the frame, simplified S BEFORE it
        if (active) {
          // phase A: alpha over the block, from its checkpoint
          const double *const r = myck + (size_t)kb * SRD;
          double aO[NL], aC[NL];
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            if (KIND == 0) {
              const double2 v = *reinterpret_cast<const double2 *>(r + lane * NS + 2 * j);
              aO[j] = v.x; aC[j] = v.y;
            } else {
              aO[j] = NINF; aC[j] = r[lane * NS + j];
            }
          }
          double acs = r[SRD - 2];
#pragma unroll
          for (int f = 0; f < F; ++f) {
            if (f < nf) {
              float e[NL];
              fused::ld_slots<NL>(rb + f * FR, e);
              const float4 sv = *reinterpret_cast<const float4 *>(sb + f * 4);
              const double Md = (double)sv.y, nl2s = -(double)sv.z;
              const double eb = fma((double)sv.x - Md, LOG2E_D, nl2s);
              auto em = [&](int j) { return fma((double)e[j] - Md, LOG2E_D, nl2s); };
              if (KIND == 0) {
                const double pO = from_prev_lane(aO[NL - 1], NINF);
                const double pC = from_prev_lane(aC[NL - 1], acs);
#pragma unroll
                for (int j = NL - 1; j >= 0; --j) {
                  const double qO = j > 0 ? aO[j > 0 ? j - 1 : 0] : pO;
                  const double qC = j > 0 ? aC[j > 0 ? j - 1 : 0] : pC;
                  const double a2 = ((allow >> j) & 1u) ? qO : NINF;
                  const double o = nb_lse(aO[j], qC, a2) + em(j);
                  aC[j] = nb_lse(aC[j], aO[j]) + eb;
                  aO[j] = o;
                }
                acs += eb;
#pragma unroll
                for (int j = 0; j < NL; ++j) { RA[f][2 * j] = aO[j]; RA[f][2 * j + 1] = aC[j]; }
                if (lane == 0) csb[wave * F + f] = acs;
              } else {
#pragma unroll
                for (int j = 0; j < NL; ++j) RA[f][j] = aC[j];
                if (lane == 0) csb[wave * F + f] = acs;
                const double pS = from_prev_lane(aC[NL - 1], acs);
#pragma unroll
                for (int j = NL - 1; j >= 0; --j) {
                  const double q = j > 0 ? aC[j > 0 ? j - 1 : 0] : pS;
                  aC[j] = nb_lse(aC[j] + eb, q + em(j));
                }
                acs += eb;
              }
            }
          }
        }
        fused::block_barrier();
        if (active) {
          // phase B: the posteriors of the block's frames, last first, and beta back over each
#pragma unroll
          for (int f = F - 1; f >= 0; --f) {
            if (f < nf) {
              float e[NL];
              fused::ld_slots<NL>(rb + f * FR, e);
              const float4 sv = *reinterpret_cast<const float4 *>(sb + f * 4);
              const double Md = (double)sv.y, nl2s = -(double)sv.z;
              const double eb = fma((double)sv.x - Md, LOG2E_D, nl2s);
              auto em = [&](int j) { return fma((double)e[j] - Md, LOG2E_D, nl2s); };
              const double Acs = csb[wave * F + f];
              float tk[NL], bl = 0.f;
              if (KIND == 0) {
#pragma unroll
                for (int j = 0; j < NL; ++j) {
                  tk[j] = post(RA[f][2 * j] + O[j]);
                  bl += post(RA[f][2 * j + 1] + C[j]);
                }
                if (lane == 0) bl += post(Acs + cs);
              } else {
                const double ap0 = from_prev_lane(RA[f][NL - 1], Acs);
#pragma unroll
                for (int j = 0; j < NL; ++j) {
                  const double ap = j > 0 ? RA[f][j > 0 ? j - 1 : 0] : ap0;
                  tk[j] = post(ap + em(j) + C[j]);
                  bl += post(RA[f][j] + eb + C[j]);
                }
                if (lane == 0) bl += post(Acs + eb + cs);
              }
              fused::st_slots<NL>(pst + f * FR + wave * UP + lane * NL, tk);
              bl = wave_sum(bl);
              if (lane == 0) bsh[f * NBEST_G + wave] = bl;
              // beta back over the frame, as MODE 2
              if (KIND == 0) {
                double x = O[0] + em(0);
                const double xl = from_next_lane(x, NINF);
                cs = nb_lse(cs + eb, x);
#pragma unroll
                for (int j = 0; j < NL; ++j) {
                  const double xn = j + 1 < NL ? O[j + 1 < NL ? j + 1 : 0] + em(j + 1 < NL ? j + 1 : 0) : xl;
                  const bool al = j + 1 < NL ? ((allow >> (j + 1)) & 1u) != 0 : allow_nx != 0;
                  const double cb = C[j] + eb;
                  O[j] = nb_lse(x, cb, al ? xn : NINF);
                  C[j] = nb_lse(cb, xn);
                  x = xn;
                }
              } else {
                double x = C[0] + em(0);
                const double xl = from_next_lane(x, NINF);
                cs = nb_lse(cs + eb, x);
#pragma unroll
                for (int j = 0; j < NL; ++j) {
                  const double xn = j + 1 < NL ? C[j + 1 < NL ? j + 1 : 0] + em(j + 1 < NL ? j + 1 : 0) : xl;
                  C[j] = nb_lse(C[j] + eb, xn);
                  x = xn;
                }
              }
            }
          }
        }
        fused::block_barrier();
      }
      fused::block_barrier();  // the group's end: the producers have written its last rows
    }
  } else {
    // ---- the producers (waves 8..11) ----
    const int tp = tid - 64 * NBEST_G, pw = wave - NBEST_G;
    unsigned long long *const bins = bins_all[pw];
    const bool wrt_logits = p.wrt == 0;
    const bool avec = (V & 3) == 0;  // (the accumulator's base is aligned)
    for (int grp = 0; grp < ngrp; ++grp) {
      const int n0 = grp * NBEST_G;
      const bool first = grp == 0, last = grp == ngrp - 1;
      unsigned goff[CNT];
      unsigned gvalid = 0;
#pragma unroll
      for (int c = 0; c < CNT; ++c) {
        const int idx = tp + NBEST_PT * c, g = idx / UP, i = idx % UP;
        bool tl;
        const int Lg = count_of(n0 + g, tl);
        const int tok = nb_token(p, (long)b * N + n0 + g, Lg, i);
        goff[c] = (unsigned)(tok >= 0 ? tok : blank) * (unsigned)esz;
        if (tok >= 0) gvalid |= 1u << c;
        tokt[idx] = tok;
      }
      float wg[NBEST_G];  // the group's weights (wavefront-uniform); 0: the hypothesis does not count and its posteriors are not read
#pragma unroll
      for (int g = 0; g < NBEST_G; ++g)
        wg[g] = n0 + g < N ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wn), n0 + g)) : 0.f;

      // the emissions of block kb into its ring buffer (past the utterance's end its last frame: never stored), its statistics
      auto gather = [&](int kb) {
        const int t0 = kb * F;
        float *const rb = ring + (kb & 1) * F * FR;
        float *const sb = stat + (kb & 1) * F * 4;
        auto frame_row = [&](int t) { return xb + (size_t)((long)(t < Tb ? t : Tb - 1) * p.xst) * esz; };
        constexpr int BATCH = 16;
#pragma unroll
        for (int k0 = 0; k0 < F * CNT; k0 += BATCH) {
          float e[BATCH];
#pragma unroll
          for (int k = 0; k < BATCH; ++k) {
            const int f = (k0 + k) / CNT, c = (k0 + k) % CNT;
            const char *const a = frame_row(t0 + f) + goff[c];
            e[k] = dt == 0 ? *reinterpret_cast<const float *>(a) : h16_to_f32(*reinterpret_cast<const unsigned short *>(a), dt);
          }
#pragma unroll
          for (int k = 0; k < BATCH; ++k) {
            const int f = (k0 + k) / CNT, c = (k0 + k) % CNT;
            if (!((gvalid >> c) & 1u)) e[k] = -__builtin_inff();
            if (t0 + f < Tb) rb[f * FR + tp + NBEST_PT * c] = e[k];
          }
        }
        if (tp < F && t0 + tp < Tb)
          *reinterpret_cast<float4 *>(sb + tp * 4) = *reinterpret_cast<const float4 *>(ws.stat + ((size_t)b * p.T + t0 + tp) * 4);
      };

      // the row stage of block kb: this wavefront's frames, out of the posterior block
      auto rowstage = [&](int kb) {
        const int t0 = kb * F;
        const int nf = Tb - t0 < F ? Tb - t0 : F;
#pragma unroll
        for (int qf = 0; qf < FPW; ++qf) {
          const int f = pw + NBEST_PW * qf;
          if (f >= nf) continue;  // (wavefront-uniform)
          const int t = t0 + f;
          const char *const x = xb + (size_t)((long)t * p.xst) * esz;
          char *const g = gb + (size_t)((long)t * p.gst) * gesz;
          float *const a = ngrp > 1 ? ws.acc + ((size_t)b * p.T + t) * V : nullptr;
          const float4 sv = *reinterpret_cast<const float4 *>(ws.stat + ((size_t)b * p.T + t) * 4);
          const float mx = sv.y, l2s = sv.z;
          float blk = 0.f;  // the blank's share: the hypotheses in their order
#pragma unroll
          for (int h = 0; h < NBEST_G; ++h)
            if (wg[h] != 0.f) blk += wg[h] * bsh[f * NBEST_G + h];
          for (int c0 = 0; c0 < V; c0 += NBG_CH) {
#pragma unroll
            for (int q = 0; q < NBG_CH / 64; ++q) bins[lane + 64 * q] = 0ull;
            wave_lds_fence();
#pragma unroll
            for (int q = 0; q < NBEST_G * NL; ++q) {
              const float w = wg[q / NL];
              if (w == 0.f) continue;
              const int idx = lane + 64 * q;
              const int tok = tokt[idx];
              const unsigned rel = (unsigned)(tok - c0);
              if (tok >= 0 && rel < (unsigned)NBG_CH)
                atomicAdd(&bins[rel], (unsigned long long)__float2ll_rn(__builtin_ldexpf(w * pst[f * FR + idx], NBG_FIX - fe)));
            }
            wave_lds_fence();
#pragma unroll
            for (int q = 0; q < NBG_CH / 256; ++q) {
              const int k = c0 + lane * 4 + 256 * q;
              if (k < V) {
                float base[4] = {0.f, 0.f, 0.f, 0.f};
                if (first) {
                  if (wrt_logits) {
                    const float4 xv = xvec ? nb_row_load4(x, k, dt) : nb_row_load4_elem(x, k, V, dt);
                    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                    for (int c = 0; c < 4; ++c) base[c] = wsum * fexp2((xs[c] - mx) * LOG2E - l2s);
                  }
                } else if (avec) {
                  const float4 av = *reinterpret_cast<const float4 *>(a + k);
                  base[0] = av.x; base[1] = av.y; base[2] = av.z; base[3] = av.w;
                } else {
#pragma unroll
                  for (int c = 0; c < 4; ++c)
                    if (k + c < V) base[c] = a[k + c];
                }
                float r[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                  const float bin = __builtin_ldexpf(__ll2float_rn((long long)bins[k - c0 + c]), fe - NBG_FIX) + (k + c == blank ? blk : 0.f);
                  r[c] = base[c] - bin;
                }
                if (last) {
                  nb_grad_put4(g, k, V, gdt, gvec, make_float4(r[0], r[1], r[2], r[3]));
                } else if (avec) {
                  *reinterpret_cast<float4 *>(a + k) = make_float4(r[0], r[1], r[2], r[3]);
                } else {
#pragma unroll
                  for (int c = 0; c < 4; ++c)
                    if (k + c < V) a[k + c] = r[c];
                }
              }
            }
            wave_lds_fence();
          }
        }
      };

      gather(nb - 1);
      fused::block_barrier();
      for (int kb = nb - 1; kb >= 0; --kb) {
        if (kb + 1 < nb) rowstage(kb + 1);
        fused::block_barrier();
        if (kb > 0) gather(kb - 1);
        fused::block_barrier();
      }
      rowstage(0);
      // the group's end: this thread's accumulator rows are in memory before the next group reads them, and nobody rewrites
      // the token table or the ring while a wavefront is still in its row stage
      __threadfence();
      fused::block_barrier();
    }
  }
}

template <int KIND, int NL, int MODE>
hipError_t launch_nbest(const Problem &p, int N, float *loss, const NbWs &ws, hipStream_t st) {
  hipLaunchKernelGGL((nbest_kernel<KIND, NL, MODE>), dim3(p.B, (N + NBEST_G - 1) / NBEST_G), dim3(NBEST_THREADS), 0, st, p, N, loss, ws);
  return hipGetLastError();
}

template <int MODE>
hipError_t run_nbest_mode(const Problem &p, int N, float *loss, const NbWs &ws, hipStream_t st) {
  typedef hipError_t Launch(const Problem &, int, float *, const NbWs &, hipStream_t);
  static Launch *const table[2][5] = {
      {launch_nbest<0, 1, MODE>, launch_nbest<0, 2, MODE>, launch_nbest<0, 4, MODE>, launch_nbest<0, 8, MODE>, launch_nbest<0, 16, MODE>},
      {launch_nbest<1, 1, MODE>, launch_nbest<1, 2, MODE>, launch_nbest<1, 4, MODE>, launch_nbest<1, 8, MODE>, launch_nbest<1, 16, MODE>}};
  const int NL = nl_for(p.U);
  const int lg = NL == 1 ? 0 : NL == 2 ? 1 : NL == 4 ? 2 : NL == 8 ? 3 : NL == 16 ? 4 : -1;
  if (lg < 0 || p.kind < 0 || p.kind > 1 || N < 1) return hipErrorInvalidValue;
  return table[p.kind][lg](p, N, loss, ws, st);
}

inline size_t nb_al(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

// The unit is compiled twice (__graft_entry__.py HIP_UNITS): as it stands for the loss and the three-launch gradient, and with
// CTC_NBEST_CKPT, and without packed float32 instructions, for the gradient from block checkpoints.
#ifndef CTC_NBEST_CKPT
size_t nbest_workspace_bytes(int, int, int, int, int, int) { return 0; }

hipError_t run_nbest(const Problem &p, int N, float *loss, hipStream_t st) { return run_nbest_mode<0>(p, N, loss, NbWs{nullptr, nullptr, nullptr}, st); }

// saved rows, then the row statistics, then log2 P: each region rounded up to 256 bytes (include/ctc_amd.h has the formula)
size_t nbest_grad_workspace_bytes(int kind, int B, int T, int, int U, int N) {
  const size_t rows = (size_t)B * N * T * nb_row_doubles(kind, 64 * nl_for(U)) * 8;
  return nb_al(rows) + nb_al((size_t)B * T * 16) + nb_al((size_t)B * N * 8);
}

hipError_t run_nbest_grad(const Problem &p, int N, const float *weight, float *loss, void *grad, char *wsp, hipStream_t st) {
  const int UP = 64 * nl_for(p.U);
  const size_t rows = nb_al((size_t)p.B * N * p.T * nb_row_doubles(p.kind, UP) * 8);
  const NbWs ws{reinterpret_cast<double *>(wsp), reinterpret_cast<float *>(wsp + rows),
                reinterpret_cast<double *>(wsp + rows + nb_al((size_t)p.B * p.T * 16))};
  if (hipError_t e = run_nbest_mode<1>(p, N, loss, ws, st)) return e;
  if (p.T == 0) return hipSuccess;  // no rows
  if (hipError_t e = run_nbest_mode<2>(p, N, loss, ws, st)) return e;
  const unsigned blocks = (unsigned)(((long)p.B * p.T + NBG_WAVES - 1) / NBG_WAVES);
  if (p.kind == 0) hipLaunchKernelGGL((nbest_grad_row_kernel<0>), dim3(blocks), dim3(64 * NBG_WAVES), 0, st, p, N, UP, weight, ws, grad);
  else hipLaunchKernelGGL((nbest_grad_row_kernel<1>), dim3(blocks), dim3(64 * NBG_WAVES), 0, st, p, N, UP, weight, ws, grad);
  return hipGetLastError();
}

#else  // CTC_NBEST_CKPT
namespace {

// the checkpointing alpha sweep (grid as every nbest_kernel launch), then one workgroup per utterance for everything else
template <int KIND, int NL>
hipError_t launch_nbest_ckpt(const Problem &p, int N, const float *weight, float *loss, void *grad, const NbWs &fw, const NbCk &bw,
                             hipStream_t st) {
  if (hipError_t e = launch_nbest<KIND, NL, 3>(p, N, loss, fw, st)) return e;
  if (p.T == 0) return hipSuccess;  // no rows
  hipLaunchKernelGGL((nbest_ckpt_bwd_kernel<KIND, NL>), dim3(p.B), dim3(NBEST_THREADS), 0, st, p, N, weight, bw, grad);
  return hipGetLastError();
}

inline bool nb_ckpt_tier(int U) { return nl_for(U) <= 4; }  // U <= 256: blocks of 16, 8 or 4 frames

}  // namespace

// checkpoints, then the row statistics, then log2 P, then the accumulator of an utterance with more than one group: each region
// rounded up to 256 bytes (include/ctc_amd.h has the formula)
size_t nbest_grad_ckpt_workspace_bytes(int kind, int B, int T, int V, int U, int N) {
  if (!nb_ckpt_tier(U)) return nbest_grad_workspace_bytes(kind, B, T, V, U, N);
  const int UP = 64 * nl_for(U), F = NBEST_RING / UP;
  const size_t ck = (size_t)B * N * ((T + F - 1) / F) * nb_row_doubles(kind, UP) * 8;
  return nb_al(ck) + nb_al((size_t)B * T * 16) + nb_al((size_t)B * N * 8) + (N > NBEST_G ? nb_al((size_t)B * T * V * 4) : 0);
}

hipError_t run_nbest_grad_ckpt(const Problem &p, int N, const float *weight, float *loss, void *grad, char *wsp, hipStream_t st) {
  if (!nb_ckpt_tier(p.U)) return run_nbest_grad(p, N, weight, loss, grad, wsp, st);
  typedef hipError_t Launch(const Problem &, int, const float *, float *, void *, const NbWs &, const NbCk &, hipStream_t);
  static Launch *const table[2][3] = {{launch_nbest_ckpt<0, 1>, launch_nbest_ckpt<0, 2>, launch_nbest_ckpt<0, 4>},
                                      {launch_nbest_ckpt<1, 1>, launch_nbest_ckpt<1, 2>, launch_nbest_ckpt<1, 4>}};
  const int NL = nl_for(p.U), UP = 64 * NL, F = NBEST_RING / UP;
  if (p.kind < 0 || p.kind > 1 || N < 1) return hipErrorInvalidValue;
  const size_t ck = nb_al((size_t)p.B * N * ((p.T + F - 1) / F) * nb_row_doubles(p.kind, UP) * 8);
  const size_t stat = nb_al((size_t)p.B * p.T * 16), logp = nb_al((size_t)p.B * N * 8);
  const NbWs fw{reinterpret_cast<double *>(wsp), reinterpret_cast<float *>(wsp + ck), reinterpret_cast<double *>(wsp + ck + stat)};
  const NbCk bw{fw.rows, fw.stat, fw.logp, N > NBEST_G ? reinterpret_cast<float *>(wsp + ck + stat + logp) : nullptr};
  return table[p.kind][NL == 1 ? 0 : NL == 2 ? 1 : 2](p, N, weight, loss, grad, fw, bw, st);
}
#endif  // CTC_NBEST_CKPT

}  // namespace ctc
