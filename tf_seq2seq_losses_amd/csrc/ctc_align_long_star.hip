// Long-form forced alignment with optional wildcards and the exclusion of the next label: ctc_amd_long_optional_wildcard_best_path
// and ctc_amd_long_star_best_path (include/ctc_amd.h), DESIGN.md section 5.31.
//
// The tiled lattice of ctc_align_long_wild.hip (label blocks x time blocks of TF frames, one launch per anti-diagonal of tiles, rows
// and columns handed over in float64, the blocked back-trace across label blocks) with the (max, +) step of ctc_align_wild.hip's OPT
// and XN kernels.  Those units stay as they are: what is file-local there is repeated here.  What is this unit's own:
//   label block      the classic OPT step at 16 positions per lane does not fit the register file, so a classic label block is
//                    UB = 512 positions, 8 per lane; the simplified one stays at 1024, 16 per lane.  The back-pointer word is 32 bits
//                    on both: classic 3 source bits per position and 8 open/closed bits, simplified 16 + 16 bits.  A ring block is
//                    one frame per producer wavefront whatever UB is, so frames_per_tile keeps its multiple of 4.
//   chain step       O'[i] = max(O[i], C[i-1], O[i-1] if allowed, C[i-2] if skip, O[i-2] if skipo) + e[i]
//                    C'[i] = max(C[i], O[i]) + x[blank]
//                    S'[i] = max(S[i] + h, S[i-1] + e[i], S[i-2] + e[i] if skip)     h = the ring slot of a wildcard, else x[blank]
//                    candidates in the order written, strict comparisons.  The mask bits are set once per tile from the labels.
//   block boundary   the states of position k UB - 1 AND of k UB - 2 before every frame: a second column buffer, written by the left
//                    block's last lane on an earlier launch, staged into LDS by the producers next to the first.  The tile's label
//                    array reaches two positions to the left (allow / skip / skipo) and one to the right (the token that a
//                    wildcard on the block's last position excludes).
//   label classes    whether a -3 is an optional wildcard or a bad label (beside another -3) is asked of the labels in global memory
//                    (star_class), so both tiles at a boundary and the trace reach one verdict.
//   row statistics   block 0's producers run the V-wide pass once per frame: (m1, k1, LSE) and, with XN, (m2, k2) through a second
//                    wave reduction.  Tiles k > 0 run on a later launch and read them.  A wildcard's ring slot holds m2 where k1 is
//                    the token it excludes, else m1; the simplified horizontal step reads the slot.
//   which tiles run  long_star_tile_active (ctc_align_long_star_plan.h): with OPT a position needs half a frame, not one.
//   back-trace       source code 3 (classic) / the second bit (simplified) moves two positions, also across a block boundary: the
//                    prefetched window of back-pointer words covers 256 positions.  The end state is the best of L - 1 and, behind
//                    an optional last position, of L - 2 (or the start state); a block whose last tile did not run is -inf.  A skipped
//                    position is reported by the trace (first = last = -1, label_score 0): it owns no frame, so the frame-parallel
//                    kernels never write it.
// Vector stores only, no atomics, one writer per element, no workgroup waits for another: the same bits on every run, and -- score's
// last bits apart -- for every frames_per_tile and batch composition.
#include "ctc_align_long_star.h"
#include "ctc_align_step.h"
#include "ctc_align_wild.h"
#include "ctc_common.h"

namespace ctc {
namespace {

constexpr int F = ALIGN_PW;   // frames per ring block: one per producer wavefront
static_assert(F == LONG_RING_FRAMES, "frames_per_tile is a multiple of the ring block");
constexpr int TRACE_BF = 64;  // frames per back-trace block: one per lane of the walking wavefront
constexpr float FLT_LOWEST = -3.402823466e38f;
constexpr int NO_INDEX = 0x7fffffff;
typedef unsigned int Word;
static_assert(sizeof(Word) == LONG_STAR_WORD_BYTES, "the plan's back-pointer word");

template <int KIND> struct Blk {
  static constexpr int NL = long_star_nl(KIND), UB = 64 * NL, RS = UB + 4, RW = long_star_row_doubles(UB);
  // lanes' words per frame in the trace window: two blocks of frames move the walk by <= 4 * TRACE_BF positions
  static constexpr int TRACE_W = (4 * TRACE_BF + 3 * NL - 1) / NL;
  static_assert((KIND == 0 ? 4 : 2) * NL == 32, "the back-pointer word is exactly full");
  static_assert((TRACE_W - 1) * NL >= 4 * TRACE_BF + NL, "the window covers the walk of two blocks");
};

struct LongStarWs {  // device pointers into the workspace (LongStarPlan offsets)
  Word *bp;
  double *col, *col2, *row, *lse;
  int *idx, *flag;
  double *mx, *mx2;  // m1, m2
  int *arg, *arg2;   // k1, k2
  double *lp;        // the sweep: LSE_t; the back-trace: lp[t, pi_t]
};

template <bool OPT> __device__ __forceinline__ bool star_is_wild(int cls) { return cls == ALIGN_WILDCARD || (OPT && cls == ALIGN_OPTIONAL); }

// The class of label position g: -1 (outside the transcript, or no emission: a bad label), a token, ALIGN_WILDCARD, or ALIGN_OPTIONAL
// for a -3 that has no -3 beside it.  Asked of the labels themselves wherever a block boundary falls.
template <bool OPT>
__device__ __forceinline__ int star_class(const Problem &p, const int32_t *lr, int g, int L) {
  if (g < 0 || g >= L) return -1;
  const int tok = label_at(p, lr, g);
  if (tok == ALIGN_WILDCARD) return tok;
  if (OPT && tok == ALIGN_OPTIONAL) {
    const bool pair = (g > 0 && label_at(p, lr, g - 1) == ALIGN_OPTIONAL) || (g + 1 < L && label_at(p, lr, g + 1) == ALIGN_OPTIONAL);
    return pair ? -1 : ALIGN_OPTIONAL;
  }
  return emits(p, tok) ? tok : -1;
}

// Running statistic of one lane (that of ctc_align_wild.hip): m = the maximum so far, idx = the lowest index holding it, s = sum of
// exp(x - max(m, FLT_LOWEST)); a lane visits its indices in ascending order, so a strict comparison keeps the lowest one
__device__ __forceinline__ void star_stat_add4(float &m, int &idx, float &s, const float4 v, int k, bool with_sum) {
  const float mo = fmaxf(m, FLT_LOWEST);
  if (v.x > m) { m = v.x; idx = k; }
  if (v.y > m) { m = v.y; idx = k + 1; }
  if (v.z > m) { m = v.z; idx = k + 2; }
  if (v.w > m) { m = v.w; idx = k + 3; }
  if (with_sum) {
    const float mn = fmaxf(m, FLT_LOWEST);
    s = s * fexp2((mo - mn) * LOG2E) +
        ((fexp2((v.x - mn) * LOG2E) + fexp2((v.y - mn) * LOG2E)) + (fexp2((v.z - mn) * LOG2E) + fexp2((v.w - mn) * LOG2E)));
  }
}
// XN: the same with the runner-up: m2 = the best element other than the one at idx, i2 = the lowest index holding it
__device__ __forceinline__ void star_stat2_add1(float &m, int &idx, float &m2, int &i2, const float v, int k) {
  const bool first = v > m, second = v > m2;
  const float nm2 = first ? m : second ? v : m2;
  const int ni2 = first ? idx : second ? k : i2;
  m2 = nm2; i2 = ni2;
  m = first ? v : m;
  idx = first ? k : idx;
}
__device__ __forceinline__ void star_stat2_add4(float &m, int &idx, float &m2, int &i2, float &s, const float4 v, int k, bool with_sum) {
  const float mo = fmaxf(m, FLT_LOWEST);
  star_stat2_add1(m, idx, m2, i2, v.x, k);
  star_stat2_add1(m, idx, m2, i2, v.y, k + 1);
  star_stat2_add1(m, idx, m2, i2, v.z, k + 2);
  star_stat2_add1(m, idx, m2, i2, v.w, k + 3);
  if (with_sum) {
    const float mn = fmaxf(m, FLT_LOWEST);
    s = s * fexp2((mo - mn) * LOG2E) +
        ((fexp2((v.x - mn) * LOG2E) + fexp2((v.y - mn) * LOG2E)) + (fexp2((v.z - mn) * LOG2E) + fexp2((v.w - mn) * LOG2E)));
  }
}

// wave-wide minimum of unsigned values, the same value in every lane (the reduction of ctc_common.h with v_min_u32)
__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
  asm(CTC_WAVE_REDUCE_ASM("v_min_u32_dpp") : "+v"(v));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// One frame of the chain for the NL positions of this lane.  fO / fC: what lane 0 takes for the position before its first, fO2 / fC2
// for the one before that -- their states BEFORE this frame (block 0: the start state and nothing before it; a block further right:
// the two columns of its left neighbour).  Returns the lane's back-pointer bits.
template <int KIND, int NL, bool OPT>
__device__ __forceinline__ Word star_chain_step(double (&O)[NL], double (&C)[NL], unsigned allow, unsigned skip, unsigned skipo,
                                                unsigned wild, double fO, double fC, double fO2, double fC2, const float (&e)[NL],
                                                double ebd) {
  const double NINF = -__builtin_inf();
  Word bits = 0;
  if (KIND == 0) {
    const double pO = from_prev_lane(O[NL - 1], fO);
    const double pC = from_prev_lane(C[NL - 1], fC);
    [[maybe_unused]] double pO2 = NINF, pC2 = NINF;
    if constexpr (OPT) {
      pO2 = from_prev_lane(O[NL - 2], fO2);
      pC2 = from_prev_lane(C[NL - 2], fC2);
    }
#pragma unroll
    for (int j = NL - 1; j >= 0; --j) {
      const double qO = j > 0 ? O[j > 0 ? j - 1 : 0] : pO;
      const double qC = j > 0 ? C[j > 0 ? j - 1 : 0] : pC;
      const double a2 = ((allow >> j) & 1u) ? qO : NINF;
      double best = O[j];
      unsigned src = 0;
      if (qC > best) { best = qC; src = 1; }
      if (a2 > best) { best = a2; src = 2; }
      if constexpr (OPT) {  // over an optional wildcard: closed i - 2, then open i - 2
        const double rC = j > 1 ? C[j > 1 ? j - 2 : 0] : j == 1 ? pC : pC2;
        const double rO = j > 1 ? O[j > 1 ? j - 2 : 0] : j == 1 ? pO : pO2;
        if (((skip >> j) & 1u) && rC > best) { best = rC; src = 3; }
        if (((skipo >> j) & 1u) && rO > best) {
          best = rO; src = 3;
          bits |= (Word)1 << (3 * NL + j);
        }
      }
      const unsigned sc = O[j] > C[j] ? 1u : 0u;
      const double bc = sc ? O[j] : C[j];
      O[j] = best + (double)e[j];
      C[j] = bc + ebd;
      bits |= (Word)(src | (sc << 2)) << (3 * j);
    }
  } else {
    const double pS = from_prev_lane(C[NL - 1], fC);
    [[maybe_unused]] double pS2 = NINF;
    if constexpr (OPT) pS2 = from_prev_lane(C[NL - 2], fC2);
#pragma unroll
    for (int j = NL - 1; j >= 0; --j) {
      const double q = j > 0 ? C[j > 0 ? j - 1 : 0] : pS;
      const double d = q + (double)e[j], h = C[j] + (((wild >> j) & 1u) ? (double)e[j] : ebd);
      const unsigned sd = d > h ? 1u : 0u;
      double best = sd ? d : h;
      if constexpr (OPT) {  // entered over an optional wildcard, from two positions back
        const double r = ((skip >> j) & 1u) ? (j > 1 ? C[j > 1 ? j - 2 : 0] : j == 1 ? pS : pS2) + (double)e[j] : NINF;
        if (r > best) {
          best = r;
          bits |= (Word)1 << (NL + j);
        }
      }
      C[j] = best;
      bits |= (Word)sd << j;
    }
  }
  return bits;
}

template <int KIND, bool OPT, bool XN>
__global__ __launch_bounds__(ALIGN_THREADS) void align_long_star_tile_kernel(const Problem p, const LongStarWs w, int K, int J, int TF,
                                                                             int d, int k_lo, int count) {
  constexpr int NL = Blk<KIND>::NL, UB = Blk<KIND>::UB, RS = Blk<KIND>::RS, RW = Blk<KIND>::RW;
  const double NINF = -__builtin_inf();
  __shared__ __attribute__((aligned(16))) float ring[2 * F * RS];
  __shared__ int lab_s[UB + 3];  // the classes (star_class) of positions k * UB - 2 .. k * UB + UB
  [[maybe_unused]] __shared__ int nx_s[XN ? UB : 1];  // XN: the token each position of the block excludes (-1: none)
  __shared__ double col_s[2][F][4];
  __shared__ double lse_s[ALIGN_PW];

  const int b = blockIdx.x / count, k = k_lo + blockIdx.x % count, j = d - k;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = p.T, V = p.V, blank = p.blank, dt = p.xdtype;
  const int Tb = frame_count(p, b);
  const int L = label_count(p, b);
  if (too_many_labels(p, L) || !long_star_tile_active(OPT, Tb, L, k, j, TF, UB)) return;
  const int t_lo = j * TF;                                   // (J * TF < T + TF: no overflow)
  const int t_hi = Tb - t_lo < TF ? Tb : t_lo + TF;          // one past the tile's last frame
  const bool fresh = long_star_fresh(OPT, k, j, TF, UB);     // the block's first tile (j == 0 included)
  const bool has_right = k + 1 < K && (k + 1) * UB < L;

  for (int i = tid; i < UB + 3; i += ALIGN_THREADS) lab_s[i] = star_class<OPT>(p, label_row(p, b), k * UB + i - 2, L);
  __syncthreads();
  if constexpr (XN) {
    for (int i = tid; i < UB; i += ALIGN_THREADS) {
      const int nt = lab_s[3 + i];
      nx_s[i] = (star_is_wild<OPT>(lab_s[2 + i]) && nt >= 0) ? nt : -1;
    }
    __syncthreads();  // (the producers read it from their first frame on)
  }

  int lab[NL];
  unsigned wild = 0;  // bit q = position k * UB + lane * NL + q is a wildcard (OPT: of either kind)
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    lab[q] = lab_s[2 + lane * NL + q];
    if (star_is_wild<OPT>(lab[q])) wild |= 1u << q;
  }

  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  // vector row accesses (16 bytes of float32, 8 bytes of 16-bit elements) need aligned rows; element-wise otherwise
  const bool vec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (dt == 0 ? 15 : 7)) == 0;
  const bool with_sum = p.wrt == 0;
  Word *const bp = w.bp + ((size_t)b * K + k) * (size_t)T * 64;
  double *const row = w.row + ((size_t)b * K + k) * RW;
  const size_t c_in = ((size_t)b * (K - 1) + (k > 0 ? k - 1 : 0)) * (size_t)T * 2, c_out = ((size_t)b * (K - 1) + k) * (size_t)T * 2;
  const double *const col_in = k > 0 ? w.col + c_in : nullptr;
  const double *const col2_in = k > 0 ? w.col2 + c_in : nullptr;
  double *const col_out = has_right ? w.col + c_out : nullptr;
  double *const col2_out = has_right ? w.col2 + c_out : nullptr;
  double *const mxw = w.mx + (size_t)b * T;
  double *const mx2w = w.mx2 + (size_t)b * T;
  int *const argw = w.arg + (size_t)b * T;
  int *const arg2w = w.arg2 + (size_t)b * T;
  double *const lpw = w.lp + (size_t)b * T;

  // chain state (wave 0): row in
  double O[NL], C[NL];  // simplified: C is S, O unused
  unsigned allow = 0;   // classic: bit q = label[i] differs from label[i-1], or one of the two is a wildcard
  // OPT: bit q of `skip` = the position before k * UB + lane * NL + q is an optional wildcard; of `skipo` = (classic) the open -> open
  // step over it is allowed
  unsigned skip = 0, skipo = 0;
  double cs = 0.0;      // the start state (label block 0): blank so far
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    O[q] = NINF; C[q] = NINF;
    const int i = lane * NL + q, g = k * UB + i;
    const int prev = lab_s[1 + i], prev2 = lab_s[i];
    if (KIND == 0 && g > 0 && (lab[q] != prev || star_is_wild<OPT>(lab[q]) || star_is_wild<OPT>(prev))) allow |= 1u << q;
    if (OPT && g >= 1 && prev == ALIGN_OPTIONAL) {
      skip |= 1u << q;
      if (KIND == 0 && g >= 2 && (lab[q] != prev2 || star_is_wild<OPT>(lab[q]) || star_is_wild<OPT>(prev2))) skipo |= 1u << q;
    }
  }
  if (wave == 0 && !fresh) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      if (KIND == 0) O[q] = row[q * 64 + lane];
      C[q] = row[(NL + q) * 64 + lane];
    }
    if (k == 0) cs = row[2 * UB];
  }
  double lse = 0.0;  // producers of block 0: sum of the LSE of this wavefront's frames

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
    const float eb = row_load1(xr, blank, dt);
    float M;
    [[maybe_unused]] float M2 = 0.f;  // XN: the best token other than k1
    [[maybe_unused]] int K1 = 0;
    if (k == 0) {
      // the row pass.  Both access paths give a lane the same elements in the same order -- c .. c+3 for c = 4 * lane, + 256, ... --
      // so their results are the same bits (an element past V enters as -inf: it never wins and adds exp(-inf) = 0)
      float m = -__builtin_inff(), s = 0.f;
      int ix = lane * 4 < V ? lane * 4 : NO_INDEX;
      [[maybe_unused]] float m2 = -__builtin_inff();  // XN: the runner-up of the lane's elements
      [[maybe_unused]] int ix2 = NO_INDEX;
      for (int c = lane * 4; c < V; c += 256) {
        float4 v;
        if (vec) {
          v = row_load4(xr, c, dt);
        } else {
          const float ninf = -__builtin_inff();
          v.x = row_load1(xr, c, dt);
          v.y = c + 1 < V ? row_load1(xr, c + 1, dt) : ninf;
          v.z = c + 2 < V ? row_load1(xr, c + 2, dt) : ninf;
          v.w = c + 3 < V ? row_load1(xr, c + 3, dt) : ninf;
        }
        if constexpr (XN) star_stat2_add4(m, ix, m2, ix2, s, v, c, with_sum);
        else star_stat_add4(m, ix, s, v, c, with_sum);
      }
      M = wave_max(m);
      // every lane whose maximum is the row's offers its lowest index; an all -inf row: every lane does, index 0 wins
      unsigned a = wave_min_u(m == M ? (unsigned)ix : (unsigned)NO_INDEX);
      if (a >= (unsigned)V) a = 0;  // (NaN rows only: unspecified, but a token of the vocabulary)
      [[maybe_unused]] unsigned a2 = 0;
      if constexpr (XN) {
        // the lane that holds k1 offers its runner-up, every other lane its own best: the best token other than k1
        const bool has = m == M && (unsigned)ix == a;
        const float cm = has ? m2 : m;
        const int ci = has ? ix2 : ix;
        M2 = wave_max(cm);
        a2 = wave_min_u(cm == M2 ? (unsigned)ci : (unsigned)NO_INDEX);
        if (a2 >= (unsigned)V) a2 = 0;  // (V = 1: there is no other token; its score is -inf)
        K1 = (int)a;
      }
      double l = 0.0;
      if (with_sum) {
        const float Mf = fmaxf(M, FLT_LOWEST);
        const float S = wave_sum(s * fexp2((fmaxf(m, FLT_LOWEST) - Mf) * LOG2E));
        l = (double)Mf + (double)flog2(S) * LN2_D;
        lse += l;
      }
      if (lane == 0) {
        mxw[t] = (double)M;
        argw[t] = (int)a;
        lpw[t] = l;
        if constexpr (XN) {
          mx2w[t] = (double)M2;
          arg2w[t] = (int)a2;
        }
      }
    } else {
      // (tile (0, j) stored them on an earlier launch; float32 values, so the round trip is exact)
      M = (float)mxw[t];
      if constexpr (XN) {
        M2 = (float)mx2w[t];
        K1 = argw[t];
      }
    }
    float *const r = ring + ((kb & 1) * F + f) * RS;
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      float v = e[q];
      if ((wild >> q) & 1u) {
        v = M;
        if constexpr (XN) {  // the best token other than the excluded one
          const int y = nx_s[lane * NL + q];
          if (y >= 0 && K1 == y) v = M2;
        }
      }
      r[lane * NL + q] = v;
    }
    if (lane == 0) r[UB] = eb;
    if (k > 0) {
      if (lane < 2) col_s[kb & 1][f][lane] = col_in[(size_t)t * 2 + lane];
      else if (OPT && lane < 4) col_s[kb & 1][f][lane] = col2_in[(size_t)t * 2 + lane - 2];
    }
  };

  auto consume = [&](int kb) {
    const int t0 = t_lo + kb * F;
    const int nf = t_hi - t0 < F ? t_hi - t0 : F;
    const float *const rb = ring + (kb & 1) * F * RS;
    float e[NL], en[NL], eb, ebn;
#pragma unroll
    for (int q = 0; q < NL; ++q) en[q] = rb[lane * NL + q];
    ebn = rb[UB];
    for (int f = 0; f < nf; ++f) {
#pragma unroll
      for (int q = 0; q < NL; ++q) e[q] = en[q];
      eb = ebn;
      {  // the next frame's emissions, one frame ahead of their use (past the block: the last row again)
        const float *const rn = rb + (f + 1 < F ? f + 1 : F - 1) * RS;
#pragma unroll
        for (int q = 0; q < NL; ++q) en[q] = rn[lane * NL + q];
        ebn = rn[UB];
      }
      const double ebd = (double)eb;
      if (col_out && lane == 63) {  // columns out: the last two positions before this frame
        const size_t at = (size_t)(t0 + f) * 2;
        col_out[at] = O[NL - 1];
        col_out[at + 1] = C[NL - 1];
        if constexpr (OPT) {
          col2_out[at] = O[NL - 2];
          col2_out[at + 1] = C[NL - 2];
        }
      }
      const double fO = k > 0 ? col_s[kb & 1][f][0] : NINF;
      const double fC = k > 0 ? col_s[kb & 1][f][1] : cs;
      const double fO2 = OPT && k > 0 ? col_s[kb & 1][f][2] : NINF;
      const double fC2 = OPT && k > 0 ? col_s[kb & 1][f][3] : NINF;
      const Word bits = star_chain_step<KIND, NL, OPT>(O, C, allow, skip, skipo, wild, fO, fC, fO2, fC2, e, ebd);
      cs += ebd;
      bp[(size_t)(t0 + f) * 64 + lane] = bits;
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

  // row out, and the block's share of the log-sum-exps
  if (wave == 0) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      row[q * 64 + lane] = O[q];
      row[(NL + q) * 64 + lane] = C[q];
    }
    if (k == 0 && lane == 0) row[2 * UB] = cs;
  } else if (lane == 0) {
    lse_s[wave - 1] = lse;
  }
  if (k == 0) {
    __syncthreads();
    if (tid == 0) w.lse[(size_t)b * J + j] = (lse_s[0] + lse_s[1]) + (lse_s[2] + lse_s[3]);
  }
}

template <int KIND, bool OPT, bool XN>
__global__ __launch_bounds__(ALIGN_THREADS) void align_long_star_trace_kernel(const Problem p, const LongStarWs w, int K, int J, int TF,
                                                                              float *__restrict__ score, int *__restrict__ tokens,
                                                                              int *__restrict__ label_index, int *__restrict__ first_frame,
                                                                              int *__restrict__ last_frame, float *__restrict__ label_score) {
  constexpr int NL = Blk<KIND>::NL, UB = Blk<KIND>::UB, RW = Blk<KIND>::RW, TRACE_W = Blk<KIND>::TRACE_W;
  const double NINF = -__builtin_inf();
  __shared__ __attribute__((aligned(16))) Word tb[2 * TRACE_BF * TRACE_W];
  __shared__ double lsum_s[64];
  __shared__ double fin_s;
  __shared__ int fin_open_s, fin_pos_s, si_s;

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = p.T, U = p.U, blank = p.blank, dt = p.xdtype;
  const int Tb = frame_count(p, b);
  const int L = label_count(p, b);
  const int32_t *const lrow = label_row(p, b);
  // a position that the path skips: an empty run (its one writer: it owns no frame)
  auto mark_skipped = [&](int pos) {
    if (first_frame) first_frame[(size_t)b * U + pos] = -1;
    if (last_frame) last_frame[(size_t)b * U + pos] = -1;
    if (label_score) label_score[(size_t)b * U + pos] = 0.f;
  };

  // ---- the end state ----
  if (wave == 0) {
    const int nj = (Tb + TF - 1) / TF;
    double s = 0.0;
    if (p.wrt == 0)
      for (int j = lane; j < nj; j += 64) s += w.lse[(size_t)b * J + j];
    lsum_s[lane] = s;
  } else if (tid == 64) {
    double best = NINF;
    int open = 0, pos = L - 1;
    const bool last_opt = OPT && L > 0 && !too_many_labels(p, L) && star_class<OPT>(p, lrow, L - 1, L) == ALIGN_OPTIONAL;
    // the states of position i after the last frame: those of its block's row buffer if the block's last tile ran, else -inf
    auto state = [&](int i, double &ov, double &cv) {
      const int kk = i / UB, r = i % UB;
      ov = NINF; cv = NINF;
      if (long_star_tile_active(OPT, Tb, L, kk, (Tb - 1) / TF, TF, UB)) {
        const double *const row = w.row + ((size_t)b * K + kk) * RW;
        if (KIND == 0) ov = row[(r % NL) * 64 + r / NL];
        cv = row[(NL + r % NL) * 64 + r / NL];
      }
    };
    if (too_many_labels(p, L) || long_star_refused(OPT, Tb, L)) {
    } else if (Tb == 0) {
      if (L == 0 || last_opt) { best = 0.0; pos = -1; }  // no frames: no labels, or one optional wildcard that stays empty
    } else if (L == 0) {
      best = w.row[(size_t)b * K * RW + 2 * UB];
    } else {
      double ov, cv;
      state(L - 1, ov, cv);
      const bool op = KIND == 0 && ov > cv;
      best = op ? ov : cv;
      open = op ? 1 : 0;
      if (last_opt) {  // the states before an optional last position: closed, then open, of L - 2 (L = 1: the start state)
        double o2 = NINF, c2;
        if (L >= 2) state(L - 2, o2, c2);
        else c2 = w.row[(size_t)b * K * RW + 2 * UB];
        if (c2 > best) { best = c2; open = 0; pos = L - 2; }
        if (o2 > best) { best = o2; open = 1; pos = L - 2; }
      }
    }
    fin_s = best;
    fin_open_s = open;
    fin_pos_s = pos;
    if (best > NINF && L > 0 && pos == L - 2) mark_skipped(L - 1);
  }
  __syncthreads();
  const double best = fin_s;
  const bool feasible = best > NINF;
  if (tid == 0) {
    double v = -__builtin_inf();
    if (feasible) {
      double s = 0.0;
      for (int q = 0; q < 64; ++q) s += lsum_s[q];
      v = best - s;
    }
    score[b] = (float)v;
    w.flag[b] = feasible ? 1 : 0;
  }
  int *const tok_out = tokens + (size_t)b * T;
  int *const idx_out = (label_index ? label_index : w.idx) + (size_t)b * T;
  for (int t = (feasible ? Tb : 0) + tid; t < T; t += ALIGN_THREADS) {
    tok_out[t] = -1;
    idx_out[t] = -1;
  }
  if (!feasible || Tb == 0) return;

  // ---- the back-trace ----
  // Blocks of TRACE_BF frames, last first.  The walk loses at most two positions per frame, so from the position at which a block
  // starts the words of the TRACE_W lanes at and below it cover that block and the one before: waves 1..4 fetch that window of the
  // previous block while wave 0 walks the current one in LDS (every lane walks the same state) and writes its outputs coalesced.
  // The walk notes a position per frame, whether the frame entered it over a skipped position and, simplified, whether the frame is
  // a horizontal step behind it: the position's class is looked up after the block, one lane per frame, off the walk's dependency chain.
  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  const int *const argw = w.arg + (size_t)b * T;
  const int *const arg2w = w.arg2 + (size_t)b * T;
  double *const lpw = w.lp + (size_t)b * T;
  const Word *const bpb = w.bp + (size_t)b * K * (size_t)T * 64;
  const int last_lane = K * 64 - 1;
  auto window = [&](int si) { const int g = si / NL - (TRACE_W - 1); return si >= 0 && g > 0 ? g : 0; };
  auto fetch = [&](int blk, int g_lo) {
    const int f0 = blk * TRACE_BF;
    const int nf = Tb - f0 < TRACE_BF ? Tb - f0 : TRACE_BF;
    Word *const dst = tb + (blk & 1) * TRACE_BF * TRACE_W;
    for (int q = tid - 64; q < nf * TRACE_W; q += ALIGN_THREADS - 64) {
      const int gl = g_lo + q % TRACE_W < last_lane ? g_lo + q % TRACE_W : last_lane;
      dst[q] = bpb[((size_t)(gl >> 6) * T + (f0 + q / TRACE_W)) * 64 + (gl & 63)];
    }
  };
  const int nblk = (Tb + TRACE_BF - 1) / TRACE_BF;
  int si = fin_pos_s, sopen = fin_open_s;  // state after the frame being decoded
  int g_cur = window(si);                  // window of the block being walked
  if (wave > 0) fetch(nblk - 1, g_cur);
  __syncthreads();
  for (int blk = nblk - 1; blk >= 0; --blk) {
    const int g_next = window(si);  // (si: where this block starts, the same in every wavefront)
    if (wave > 0) {
      if (blk > 0) fetch(blk - 1, g_next);
    } else {
      const int f0 = blk * TRACE_BF;
      const int nf = Tb - f0 < TRACE_BF ? Tb - f0 : TRACE_BF;
      const Word *const wd = tb + (blk & 1) * TRACE_BF * TRACE_W;
      int mypos = -1, myflags = 0;  // bit 0: a horizontal step, bit 1: entered over a skipped position
      for (int fl = nf - 1; fl >= 0; --fl) {
        int pos = -1, flags = 0;
        if (si >= 0) {
          const Word word = wd[fl * TRACE_W + (si / NL - g_cur)];
          const int q = si & (NL - 1);
          if (KIND == 0) {
            const unsigned c = (word >> (3 * q)) & 7u;
            if (sopen) {
              pos = si;
              const unsigned src = c & 3u;
              if (src == 1) { --si; sopen = 0; }
              else if (src == 2) --si;
              else if (OPT && src == 3) {  // over an optional wildcard: the spare bit says which state two back
                sopen = (int)((word >> (3 * NL + q)) & 1u);
                si -= 2;
                flags = 2;
              }
            } else if (c & 4u) {
              sopen = 1;
            }
          } else if (OPT && ((word >> (NL + q)) & 1u)) {  // entered from two back (it outranks bit q)
            pos = si;
            si -= 2;
            flags = 2;
          } else if ((word >> q) & 1u) {
            pos = si;
            --si;
          } else {  // a horizontal step behind position si: the wildcard's frame if si is one, a blank otherwise
            pos = si;
            flags = 1;
          }
          if (si < 0) sopen = 0;
        }
        if (lane == fl) { mypos = pos; myflags = flags; }
      }
      if (lane < nf) {
        const int t = f0 + lane;
        int tok = blank, idx = -1;
        if (mypos >= 0) {
          const int cls = star_class<OPT>(p, lrow, mypos, L);
          if (star_is_wild<OPT>(cls)) {
            tok = argw[t];
            idx = mypos;
            if constexpr (XN) {  // the token that was scored: k1 unless the position excludes it
              const int nt = star_class<OPT>(p, lrow, mypos + 1, L);
              if (nt >= 0 && tok == nt) tok = arg2w[t];
            }
          } else if (!(myflags & 1)) {
            tok = cls;
            idx = mypos;
          }
          if ((myflags & 2) && mypos >= 1) mark_skipped(mypos - 1);
        }
        tok_out[t] = tok;
        idx_out[t] = idx;
        // (a feasible path emits tokens of the vocabulary only; the guard keeps the read inside the row whatever the inputs hold)
        lpw[t] = (double)row_load1(xb + (size_t)((long)t * p.xst) * esz, in_vocab(p, tok) ? tok : blank, dt) - lpw[t];  // (log-probability input: LSE_t = 0)
      }
      if (lane == 0) si_s = si;
    }
    __syncthreads();
    si = si_s;
    g_cur = g_next;
    __syncthreads();  // (si_s is written again in the next round)
  }
}

// first_frame / last_frame from label_index (the kernel of ctc_align_long_wild.hip): thread n looks at frame n (a label's first frame
// is the one whose predecessor shows another index, its last the one whose successor does: one writer per element) and at label
// position n (-1 from label_length on and for an infeasible utterance; a skipped position of a feasible one is the trace's)
__global__ __launch_bounds__(256) void align_long_star_frames_kernel(const Problem p, const int *__restrict__ idx,
                                                                     const int *__restrict__ flag, int per_b,
                                                                     int *__restrict__ first_frame, int *__restrict__ last_frame) {
  const int b = blockIdx.x / per_b, n = (blockIdx.x % per_b) * 256 + threadIdx.x;
  const int T = p.T, U = p.U;
  const int Tb = frame_count(p, b), L = label_count(p, b);
  const bool feasible = flag[b] != 0;
  if (n < U && (!feasible || n >= L)) {
    if (first_frame) first_frame[(size_t)b * U + n] = -1;
    if (last_frame) last_frame[(size_t)b * U + n] = -1;
  }
  if (feasible && n < Tb) {
    const int *const row = idx + (size_t)b * T;
    const int i = row[n];
    if (i >= 0 && i < U) {
      if (first_frame && (n == 0 || row[n - 1] != i)) first_frame[(size_t)b * U + i] = n;
      if (last_frame && (n + 1 == Tb || row[n + 1] != i)) last_frame[(size_t)b * U + i] = n;
    }
  }
}

// label_score from label_index and lp[t, pi_t] (the kernel of ctc_align_long_wild.hip): thread n looks at frame n; where it is the
// first frame of label i the thread is that label's one writer and adds up the label's frames -- contiguous on both lattices -- in
// time order in float64, eight loads in flight at a time.  ... and at label position n: -inf from label_length on and for an
// infeasible utterance.
__global__ __launch_bounds__(256) void align_long_star_score_kernel(const Problem p, const int *__restrict__ idx,
                                                                    const int *__restrict__ flag, const double *__restrict__ lp,
                                                                    int per_b, float *__restrict__ label_score) {
  const int b = blockIdx.x / per_b, n = (blockIdx.x % per_b) * 256 + threadIdx.x;
  const int T = p.T, U = p.U;
  const int Tb = frame_count(p, b), L = label_count(p, b);
  const bool feasible = flag[b] != 0;
  if (n < U && (!feasible || n >= L)) label_score[(size_t)b * U + n] = -__builtin_inff();
  if (feasible && n < Tb) {
    const int *const row = idx + (size_t)b * T;
    const double *const lpr = lp + (size_t)b * T;
    const int i = row[n];
    if (i >= 0 && i < U && (n == 0 || row[n - 1] != i)) {
      double s = 0.0;
      bool more = true;
      for (int t = n; more; t += 8) {
        int ii[8];
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int tt = t + q < Tb ? t + q : Tb - 1;  // (past the end: a valid frame, dropped)
          ii[q] = t + q < Tb ? row[tt] : -1;
          v[q] = lpr[tt];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          more = more && ii[q] == i;
          if (more) s += v[q];
        }
      }
      label_score[(size_t)b * U + i] = (float)s;
    }
  }
}

template <int KIND, bool OPT, bool XN>
void launch_long_star(const Problem &p, const LongStarPlan &S, const LongStarWs &w, float *score, int *tokens, int *label_index,
                      int *first_frame, int *last_frame, float *label_score, hipStream_t st) {
  const LongPlan &P = S.base;
  if (p.T > 0) {
    for (int d = 0; d < P.launches; ++d) {
      int k_lo, count;
      long_diagonal(P, d, &k_lo, &count);
      hipLaunchKernelGGL((align_long_star_tile_kernel<KIND, OPT, XN>), dim3((unsigned)((size_t)p.B * count)), dim3(ALIGN_THREADS), 0, st, p,
                         w, P.K, P.J, P.TF, d, k_lo, count);
    }
  }
  hipLaunchKernelGGL((align_long_star_trace_kernel<KIND, OPT, XN>), dim3(p.B), dim3(ALIGN_THREADS), 0, st, p, w, P.K, P.J, P.TF, score,
                     tokens, label_index, first_frame, last_frame, label_score);
}

}  // namespace

hipError_t run_align_long_star(const Problem &p, const LongStarPlan &S, char *ws, float *score, int *tokens, int *label_index,
                               int *first_frame, int *last_frame, float *label_score, hipStream_t st, bool optional_wildcards,
                               bool exclude_next_label) {
  if (p.kind < 0 || p.kind > 1 || S.UB != long_star_block(p.kind) || !(optional_wildcards || exclude_next_label)) return hipErrorInvalidValue;
  const LongPlan &P = S.base;
  LongStarWs w;
  w.bp = reinterpret_cast<Word *>(ws + P.off_bp);
  w.col = reinterpret_cast<double *>(ws + P.off_col);
  w.col2 = reinterpret_cast<double *>(ws + S.off_col2);
  w.row = reinterpret_cast<double *>(ws + P.off_row);
  w.lse = reinterpret_cast<double *>(ws + P.off_lse);
  w.idx = reinterpret_cast<int *>(ws + P.off_idx);
  w.flag = reinterpret_cast<int *>(ws + P.off_flag);
  w.mx = reinterpret_cast<double *>(ws + S.off_max);
  w.mx2 = reinterpret_cast<double *>(ws + S.off_max2);
  w.arg = reinterpret_cast<int *>(ws + S.off_arg);
  w.arg2 = reinterpret_cast<int *>(ws + S.off_arg2);
  w.lp = reinterpret_cast<double *>(ws + S.off_lp);
  typedef void Launch(const Problem &, const LongStarPlan &, const LongStarWs &, float *, int *, int *, int *, int *, float *, hipStream_t);
  static Launch *const table[2][3] = {{launch_long_star<0, true, false>, launch_long_star<0, false, true>, launch_long_star<0, true, true>},
                                      {launch_long_star<1, true, false>, launch_long_star<1, false, true>, launch_long_star<1, true, true>}};
  table[p.kind][optional_wildcards ? (exclude_next_label ? 2 : 0) : 1](p, S, w, score, tokens, label_index, first_frame, last_frame,
                                                                      label_score, st);
  const int per_b = ((p.T > p.U ? p.T : p.U) + 255) / 256;
  const int *const idx = label_index ? label_index : w.idx;
  if ((first_frame || last_frame) && per_b > 0)
    hipLaunchKernelGGL(align_long_star_frames_kernel, dim3((unsigned)((size_t)p.B * per_b)), dim3(256), 0, st, p, idx, w.flag, per_b,
                       first_frame, last_frame);
  if (label_score && per_b > 0)
    hipLaunchKernelGGL(align_long_star_score_kernel, dim3((unsigned)((size_t)p.B * per_b)), dim3(256), 0, st, p, idx, w.flag, w.lp,
                       per_b, label_score);
  return hipGetLastError();
}

}  // namespace ctc
