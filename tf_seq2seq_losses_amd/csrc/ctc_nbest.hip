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
    double *const myrows = MODE != 0 ? ws.rows + (size_t)hrow * p.T * SRD : nullptr;  // (n >= N: never dereferenced)
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
        if (MODE == 1) ws.logp[hrow] = v;
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
          if (MODE == 1 && blockIdx.y == 0) *reinterpret_cast<float4 *>(ws.stat + ((size_t)b * p.T + t0 + f) * 4) = make_float4(ebl[q], M, l2s, 0.f);
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

}  // namespace ctc
