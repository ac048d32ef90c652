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

template <int KIND, int NL>
__global__ __launch_bounds__(NBEST_THREADS) void nbest_kernel(const Problem p, const int N, float *__restrict__ loss) {
  constexpr int UP = 64 * NL;
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
      }
    };

    fused::block_barrier();
    for (int kb = 0; kb < nb; ++kb) {
      if (n < N) consume(kb);
      fused::block_barrier();
    }

    // the end state
    if (n < N) {
      const int i = L - 1, jj = i & (NL - 1);
      double cv = C[0], ov = O[0];
#pragma unroll
      for (int j = 1; j < NL; ++j)
        if (j == jj) { cv = C[j]; ov = O[j]; }
      double v = cs;
      if (L > 0) v = KIND == 0 ? nb_lse(ov, cv) : cv;
      if (too_long) v = NINF;
      if (lane == (L > 0 ? i / NL : 0)) loss[hrow] = (float)(0.0 - v * LN2_D);  // (-inf: +inf; an empty utterance: +0)
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
    // row t of the utterance; past its end the last row, valid memory whose results are never stored
    auto frame_row = [&](int t) { return xb + (size_t)((long)(t < Tb ? t : Tb - 1) * p.xst) * esz; };

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
        const int t = (f < F && t0 + f < Tb) ? t0 + f : Tb - 1;
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
        if (lane == 0 && f < F && t0 + f < Tb) *reinterpret_cast<float4 *>(sb + f * 4) = make_float4(ebl[q], M, l2s, 0.f);
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

template <int KIND, int NL>
hipError_t launch_nbest(const Problem &p, int N, float *loss, hipStream_t st) {
  hipLaunchKernelGGL((nbest_kernel<KIND, NL>), dim3(p.B, (N + NBEST_G - 1) / NBEST_G), dim3(NBEST_THREADS), 0, st, p, N, loss);
  return hipGetLastError();
}

}  // namespace

size_t nbest_workspace_bytes(int, int, int, int, int, int) { return 0; }

hipError_t run_nbest(const Problem &p, int N, float *loss, hipStream_t st) {
  typedef hipError_t Launch(const Problem &, int, float *, hipStream_t);
  static Launch *const table[2][5] = {
      {launch_nbest<0, 1>, launch_nbest<0, 2>, launch_nbest<0, 4>, launch_nbest<0, 8>, launch_nbest<0, 16>},
      {launch_nbest<1, 1>, launch_nbest<1, 2>, launch_nbest<1, 4>, launch_nbest<1, 8>, launch_nbest<1, 16>}};
  const int NL = nl_for(p.U);
  const int lg = NL == 1 ? 0 : NL == 2 ? 1 : NL == 4 ? 2 : NL == 8 ? 3 : NL == 16 ? 4 : -1;
  if (lg < 0 || p.kind < 0 || p.kind > 1 || N < 1) return hipErrorInvalidValue;
  return table[p.kind][lg](p, N, loss, st);
}

}  // namespace ctc
