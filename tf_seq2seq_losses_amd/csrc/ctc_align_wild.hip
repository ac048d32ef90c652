// Forced alignment of partial transcripts: best path with wildcard labels on both CTC lattices: ctc_amd_wildcard_best_path
// (include/ctc_amd.h), DESIGN.md section 5.15.
//
// The decomposition, the float64 (max, +) chain on the raw inputs, the back-pointer words and the blocked back-trace of
// ctc_align.hip (which stays as it is: its file-local helpers are repeated here).  A label equal to ALIGN_WILDCARD marks a wildcard
// position: any non-empty run of frames with any tokens on them, worth sum_t m_t with m_t = max_k x[t, k], reported as
// a_t = the lowest k that attains it.  What differs from ctc_align.hip:
//   producers   one pass over every row for (max, lowest index at the max, sum of exp) -- for log-probability input too, without
//               the sum.  The emission of a wildcard position is m_t: the producer writes it into that position's ring slot, so
//               the chain reads its emissions as before.  m_t also goes beside the blank's emission in the ring row (slot UP + 1),
//               a_t and the frame's log-sum-exp go to the workspace.
//   chain       classic: the step from an open position straight into the next open one is allowed on both sides of a wildcard
//               (two more bits of `allow`, set once).  Simplified: while S[i] of a wildcard is the current state the horizontal step
//               costs m_t instead of x[t, blank] (one select per position).  Nothing transcendental.
//     O'[i] = max(O[i], C[i-1], O[i-1] if label[i] != label[i-1] or either is a wildcard) + e[i]     e[i] = m_t for a wildcard
//     C'[i] = max(C[i], O[i]) + x[blank]
//     S'[i] = max(S[i] + (m_t if i is a wildcard else x[blank]), S[i-1] + e[i])
//   back-trace  writes a_t on wildcard frames (classic: the open state of a wildcard; simplified: its entry and every horizontal
//               step behind it), turns the workspace's log-sum-exp of every frame into the log-probability of the path's token
//               and notes the first and last frame of every label in LDS.  Each label's frames are contiguous on both lattices:
//               afterwards one lane per label sums its own range in time order in float64.
// WIN (ctc_amd_windowed_best_path): every lane holds the (first, last) frames of its own NL positions and the
// producers write -inf for a position whose frame lies outside them -- a wildcard's m_t included, so on the simplified lattice the
// horizontal step behind a wildcard costs its ring slot instead of the wave-uniform m_t.  Nothing behind the ring knows of windows.
// OPT (ctc_amd_optional_wildcard_best_path): a label equal to ALIGN_OPTIONAL is a wildcard position that may be
// skipped.  Two mask bits per position, set once (`skip`: the position before me is optional; `skipo`: classic, the open -> open
// step over it is allowed) add two candidates to the open state, behind the existing ones and with strict comparisons too:
//     O'[i] = max(O[i], C[i-1], O[i-1] if allowed, C[i-2] if skip, O[i-2] if skipo) + e[i]     (position -1 is the start state)
//     S'[i] = max(S[i] + h, S[i-1] + e[i], S[i-2] + e[i] if skip)
// The state two positions back comes from the lane's own registers or by one more DPP shift.  Back-pointers fit the same words:
// classic, source code 3 of the open state = "two back" and the spare bit 3 NL + j says closed (0) or open (1); simplified, a second
// bit NL + j = "entered from two back".  A last optional position makes the states before it end states (candidates in the order
// closed, open of L - 1, then closed, open of L - 2 or the start state).  A skipped position reports first = last = -1 and a
// label_score of 0, the log-probability of an empty run.
// Every output element has one writer, no atomics: the same bits on every run.
#include <type_traits>

#include "ctc_align_wild.h"
#include "ctc_common.h"

namespace ctc {
namespace {

constexpr int ALIGN_PW = 4;                         // producer wavefronts
constexpr int ALIGN_THREADS = 64 * (1 + ALIGN_PW);  // + the chain
constexpr int ALIGN_RING = 4096;                    // label emissions per ring buffer (two buffers): frames per block = 4096 / UP
constexpr float FLT_LOWEST = -3.402823466e38f;
constexpr int NO_INDEX = 0x7fffffff;

// back-pointer word of one lane and frame: 3 bits per label position (classic; simplified uses 1), NL positions
template <int NL> struct BpWord { typedef unsigned char type; };
template <> struct BpWord<4> { typedef unsigned short type; };
template <> struct BpWord<8> { typedef unsigned int type; };
template <> struct BpWord<16> { typedef unsigned long long type; };

constexpr int bp_word_bytes(int NL) { return NL <= 2 ? 1 : NL / 2; }
// frames per back-trace block: two blocks of (frames x 64 lanes x word) fit the LDS the ring used (32 KB)
constexpr int trace_frames(int NL) { return NL == 16 ? 32 : 64; }
constexpr size_t r256(size_t x) { return (x + 255) & ~size_t(255); }

// elements k .. k+3 of a row of element type dt (0 = float32, 1 = bfloat16, 2 = float16) as float32 (row_load1: ctc_common.h)
__device__ __forceinline__ float4 row_load4(const char *row, int k, int dt) {
  if (dt == 0) return *reinterpret_cast<const float4 *>(row + (size_t)k * 4);
  const uint2 u = *reinterpret_cast<const uint2 *>(row + (size_t)k * 2);
  return make_float4(h16_to_f32((unsigned short)(u.x & 0xffffu), dt), h16_to_f32((unsigned short)(u.x >> 16), dt),
                     h16_to_f32((unsigned short)(u.y & 0xffffu), dt), h16_to_f32((unsigned short)(u.y >> 16), dt));
}

// Running statistic of one lane (that of ctc_decode.hip): m = the maximum so far (-inf before the first element), idx = the lowest
// index holding it, s = sum of exp(x - max(m, FLT_LOWEST)) (the clamp keeps -inf elements and all -inf rows free of inf - inf).  A
// lane visits its indices in ascending order, so a strict comparison keeps the lowest one.  with_sum == false (log-probability
// input; the same in every lane): no sum is needed.
__device__ __forceinline__ void stat_add4(float &m, int &idx, float &s, const float4 v, int k, bool with_sum) {
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

// wave-wide minimum of unsigned values, the same value in every lane (the reduction of ctc_common.h with v_min_u32)
__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
  asm(CTC_WAVE_REDUCE_ASM("v_min_u32_dpp") : "+v"(v));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

template <int KIND, int NL, bool WIN, bool OPT>
__global__ __launch_bounds__(ALIGN_THREADS) void align_wild_kernel(const Problem p, char *__restrict__ ws, size_t off_lp, size_t off_at,
                                                                   float *__restrict__ score, int *__restrict__ tokens,
                                                                   int *__restrict__ label_index, int *__restrict__ first_frame,
                                                                   int *__restrict__ last_frame, float *__restrict__ label_score,
                                                                   const int32_t *__restrict__ win, int wstride) {
  static_assert(!(WIN && OPT), "frame windows and optional wildcards are not combined");
  typedef typename BpWord<NL>::type Word;
  typedef typename std::conditional<NL == 16, unsigned long long, unsigned int>::type Bits;
  constexpr int UP = 64 * NL;
  constexpr int F = ALIGN_RING / UP;                 // frames per ring buffer: 64, 32, 16, 8, 4
  constexpr int RS = UP + 4;                         // ring row: UP label emissions, then the blank's, then the row maximum
  constexpr int FPW = F / ALIGN_PW;                  // frames per producer wavefront and block
  constexpr int G = FPW < 4 ? FPW : 4;               // ... of which G are in flight together
  constexpr int BF = trace_frames(NL);
  constexpr int RING_BYTES = 2 * F * RS * 4, TRACE_BYTES = 2 * BF * 64 * (int)sizeof(Word);
  constexpr int SMEM = RING_BYTES > TRACE_BYTES ? RING_BYTES : TRACE_BYTES;
  const double NINF = -__builtin_inf();

  __shared__ __attribute__((aligned(16))) char smem[SMEM];  // the ring during the sweep, back-pointer blocks during the back-trace
  __shared__ int lab_s[UP];                                  // validated labels (-1: no emission, ALIGN_WILDCARD: a wildcard)
  __shared__ int first_s[UP], last_s[UP];                    // first and last frame of every label on the path
  __shared__ double lse_s[ALIGN_PW];
  __shared__ double fin_s;
  __shared__ int fin_open_s;
  [[maybe_unused]] __shared__ int fin_pos_s;  // OPT: the end state's position, L - 1 or L - 2 (-1: the start state)
  float *const ring = reinterpret_cast<float *>(smem);

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = p.T, V = p.V, U = p.U, blank = p.blank, dt = p.xdtype;
  const int Tb = frame_count(p, b);
  int L = label_count(p, b);
  const bool too_long = too_many_labels(p, L);
  if (too_long) L = 0;  // (nothing of such an utterance is read; it is reported infeasible below)

  for (int i = tid; i < UP; i += ALIGN_THREADS) {
    int tok = -1;
    if (i < L) tok = label_at(p, label_row(p, b), i);
    lab_s[i] = tok == ALIGN_WILDCARD || (OPT && tok == ALIGN_OPTIONAL) ? tok : emits(p, tok) ? tok : -1;
    first_s[i] = -1; last_s[i] = -1;
  }
  __syncthreads();
  auto is_wild = [](int tok) { return tok == ALIGN_WILDCARD || (OPT && tok == ALIGN_OPTIONAL); };
  [[maybe_unused]] bool last_opt = false;  // OPT: the last position is optional: the states before it are end states too
  if constexpr (OPT) {  // an optional wildcard beside another one is a bad label: no emission, no skip
    bool pair[(UP + ALIGN_THREADS - 1) / ALIGN_THREADS];
#pragma unroll
    for (int q = 0; q < (UP + ALIGN_THREADS - 1) / ALIGN_THREADS; ++q) {
      const int i = tid + q * ALIGN_THREADS;
      pair[q] = i < UP && lab_s[i] == ALIGN_OPTIONAL &&
                ((i > 0 && lab_s[i - 1] == ALIGN_OPTIONAL) || (i + 1 < UP && lab_s[i + 1] == ALIGN_OPTIONAL));
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < (UP + ALIGN_THREADS - 1) / ALIGN_THREADS; ++q)
      if (pair[q]) lab_s[tid + q * ALIGN_THREADS] = -1;
    __syncthreads();
    last_opt = L > 0 && lab_s[L - 1] == ALIGN_OPTIONAL;
  }

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
  Word *const bp = reinterpret_cast<Word *>(ws) + (size_t)b * T * 64;
  double *const lpw = reinterpret_cast<double *>(ws + off_lp) + (size_t)b * T;  // the sweep: LSE_t; the back-trace: lp[t, pi_t]
  int *const atw = reinterpret_cast<int *>(ws + off_at) + (size_t)b * T;        // a_t

  // ---- the sweep ----
  // chain state (wave 0)
  double O[NL], C[NL];  // simplified: C is S, O unused
  unsigned allow = 0;   // classic: bit j = label[i] differs from label[i-1], or one of the two is a wildcard
  double cs = 0.0;      // the start state: blank so far
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    O[j] = NINF; C[j] = NINF;
    const int i = lane * NL + j;
    if (KIND == 0 && i > 0) {
      const int prev = lab_s[i - 1];
      if (lab[j] != prev || is_wild(lab[j]) || is_wild(prev)) allow |= 1u << j;
    }
  }
  // OPT: bit j of `skip` = the position before lane * NL + j is an optional wildcard; of `skipo` = (classic) the open -> open step
  // over it is allowed
  [[maybe_unused]] unsigned skip = 0, skipo = 0;
  if constexpr (OPT) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int i = lane * NL + j;
      if (i >= 1 && lab_s[i - 1] == ALIGN_OPTIONAL) {
        skip |= 1u << j;
        if (KIND == 0 && i >= 2 && (lab[j] != lab_s[i - 2] || is_wild(lab[j]) || is_wild(lab_s[i - 2]))) skipo |= 1u << j;
      }
    }
  }
  double lse = 0.0;  // producers: sum of the LSE of this wavefront's frames

  const bool with_sum = p.wrt == 0;
  auto produce = [&](int kb) {
    const int pw = wave - 1, t0 = kb * F;
    float *const rb = ring + (kb & 1) * F * RS;
    for (int f0 = pw * FPW; f0 < (pw + 1) * FPW; f0 += G) {
      if (t0 + f0 >= Tb) break;
      const char *row[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int t = t0 + f0 + g < Tb ? t0 + f0 + g : Tb - 1;  // (past the end: a valid row, its results are dropped)
        row[g] = xb + (size_t)((long)t * p.xst) * esz;
      }
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
      // the row pass.  Both access paths give a lane the same elements in the same order -- k .. k+3 for k = 4 * lane, + 256, ... --
      // so their results are the same bits (an element past V enters as -inf: it never wins and adds exp(-inf) = 0)
      float m[G], s[G];
      int ix[G];
#pragma unroll
      for (int g = 0; g < G; ++g) { m[g] = -__builtin_inff(); s[g] = 0.f; ix[g] = lane * 4 < V ? lane * 4 : NO_INDEX; }
      for (int k = lane * 4; k < V; k += 256) {
        float4 v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (vec) {
            v[g] = row_load4(row[g], k, dt);
          } else {
            const float ninf = -__builtin_inff();
            v[g].x = row_load1(row[g], k, dt);
            v[g].y = k + 1 < V ? row_load1(row[g], k + 1, dt) : ninf;
            v[g].z = k + 2 < V ? row_load1(row[g], k + 2, dt) : ninf;
            v[g].w = k + 3 < V ? row_load1(row[g], k + 3, dt) : ninf;
          }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) stat_add4(m[g], ix[g], s[g], v[g], k, with_sum);
      }
      float M[G];
      int my_a = 0;
      double my_lse = 0.0;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        M[g] = wave_max(m[g]);
        // every lane whose maximum is the row's offers its lowest index; an all -inf row: every lane does, index 0 wins
        unsigned a = wave_min_u(m[g] == M[g] ? (unsigned)ix[g] : (unsigned)NO_INDEX);
        if (a >= (unsigned)V) a = 0;  // (NaN rows only: unspecified, but a token of the vocabulary)
        double l = 0.0;
        if (with_sum) {
          const float Mf = fmaxf(M[g], FLT_LOWEST);
          const float S = wave_sum(s[g] * fexp2((fmaxf(m[g], FLT_LOWEST) - Mf) * LOG2E));
          l = (double)Mf + (double)flog2(S) * LN2_D;
          if (t0 + f0 + g < Tb) lse += l;
        }
        if (lane == g) { my_a = (int)a; my_lse = l; }
      }
      if (lane < G && t0 + f0 + lane < Tb) {
        atw[t0 + f0 + lane] = my_a;
        lpw[t0 + f0 + lane] = my_lse;
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (t0 + f0 + g < Tb) {
          float *const r = rb + (f0 + g) * RS;
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            float v = ((wild >> j) & 1u) ? M[g] : e[g][j];
            if constexpr (WIN) {
              if (t0 + f0 + g < wf[j] || t0 + f0 + g > wl[j]) v = -__builtin_inff();
            }
            r[lane * NL + j] = v;
          }
          if (lane == 0) { r[UP] = eb[g]; r[UP + 1] = M[g]; }
        }
      }
    }
  };

  auto consume = [&](int kb) {
    const int t0 = kb * F;
    const int nf = Tb - t0 < F ? Tb - t0 : F;
    const float *const rb = ring + (kb & 1) * F * RS;
    float e[NL], en[NL], eb, ebn, em = 0.f, emn = 0.f;
#pragma unroll
    for (int j = 0; j < NL; ++j) en[j] = rb[lane * NL + j];
    ebn = rb[UP];
    if (KIND == 1) emn = rb[UP + 1];
    for (int f = 0; f < nf; ++f) {
#pragma unroll
      for (int j = 0; j < NL; ++j) e[j] = en[j];
      eb = ebn; em = emn;
      {  // the next frame's emissions, one frame ahead of their use (past the block: the last row again)
        const float *const rn = rb + (f + 1 < F ? f + 1 : F - 1) * RS;
#pragma unroll
        for (int j = 0; j < NL; ++j) en[j] = rn[lane * NL + j];
        ebn = rn[UP];
        if (KIND == 1) emn = rn[UP + 1];
      }
      const double ebd = (double)eb;
      Bits bits = 0;
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
              bits |= (Bits)1 << (3 * NL + j);
            }
          }
          const unsigned sc = O[j] > C[j] ? 1u : 0u;
          const double bc = sc ? O[j] : C[j];
          O[j] = best + (double)e[j];
          C[j] = bc + ebd;
          bits |= (Bits)(src | (sc << 2)) << (3 * j);
        }
      } else {
        const double emd = (double)em;
        const double pS = from_prev_lane(C[NL - 1], cs);
        [[maybe_unused]] double pS2 = NINF;
        if constexpr (OPT) pS2 = from_prev_lane(NL == 1 ? pS : C[NL > 1 ? NL - 2 : 0], NINF);
#pragma unroll
        for (int j = NL - 1; j >= 0; --j) {
          const double q = j > 0 ? C[j > 0 ? j - 1 : 0] : pS;
          const double d = q + (double)e[j], h = C[j] + (((wild >> j) & 1u) ? (WIN ? (double)e[j] : emd) : ebd);
          const unsigned sd = d > h ? 1u : 0u;
          double best = sd ? d : h;
          if constexpr (OPT) {  // entered over an optional wildcard, from two positions back
            const double r = ((skip >> j) & 1u) ? (j > 1 ? C[j > 1 ? j - 2 : 0] : j == 1 ? pS : pS2) + (double)e[j] : NINF;
            if (r > best) {
              best = r;
              bits |= (Bits)1 << (NL + j);
            }
          }
          C[j] = best;
          bits |= (Bits)sd << j;
        }
      }
      cs += ebd;
      bp[(size_t)(t0 + f) * 64 + lane] = (Word)bits;
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

  // ---- the end state ----
  if (wave == 0) {
    const int i = L - 1, jj = i & (NL - 1);
    double cv = C[0], ov = O[0];
#pragma unroll
    for (int j = 1; j < NL; ++j)
      if (j == jj) { cv = C[j]; ov = O[j]; }
    if (L == 0) {
      if (lane == 0) {
        fin_s = cs; fin_open_s = 0;
        if constexpr (OPT) fin_pos_s = -1;
      }
    } else {
      [[maybe_unused]] double c2 = NINF, o2 = NINF;  // OPT: the states of position L - 2 (L = 1: the start state), in every lane
      if constexpr (OPT) {
        if (last_opt) {
          const int i2 = L >= 2 ? L - 2 : 0, j2 = i2 & (NL - 1);
          c2 = C[0]; o2 = O[0];
#pragma unroll
          for (int j = 1; j < NL; ++j)
            if (j == j2) { c2 = C[j]; o2 = O[j]; }
          c2 = __shfl(c2, i2 / NL);
          o2 = KIND == 0 ? __shfl(o2, i2 / NL) : NINF;
          if (L == 1) { c2 = cs; o2 = NINF; }
        }
      }
      if (lane == i / NL) {
        const bool op = KIND == 0 && ov > cv;
        double fin = op ? ov : cv;
        int fopen = op ? 1 : 0, fpos = L - 1;
        if constexpr (OPT) {
          if (c2 > fin) { fin = c2; fopen = 0; fpos = L - 2; }
          if (o2 > fin) { fin = o2; fopen = 1; fpos = L - 2; }
        }
        fin_s = fin; fin_open_s = fopen;
        if constexpr (OPT) fin_pos_s = fpos;
      }
    }
  } else if (lane == 0) {
    lse_s[wave - 1] = lse;
  }
  __syncthreads();
  const double best = fin_s;
  const bool feasible = !too_long && best > NINF;
  if (tid == 0) {
    double v = -__builtin_inf();
    if (feasible) v = p.wrt == 0 ? best - ((lse_s[0] + lse_s[1]) + (lse_s[2] + lse_s[3])) : best;
    score[b] = (float)v;
  }
  int *const tok_out = tokens + (size_t)b * T;
  int *const idx_out = label_index ? label_index + (size_t)b * T : nullptr;
  int *const first_out = first_frame ? first_frame + (size_t)b * U : nullptr;
  int *const last_out = last_frame ? last_frame + (size_t)b * U : nullptr;
  float *const ls_out = label_score ? label_score + (size_t)b * U : nullptr;
  for (int t = (feasible ? Tb : 0) + tid; t < T; t += ALIGN_THREADS) {
    tok_out[t] = -1;
    if (idx_out) idx_out[t] = -1;
  }
  if (!feasible || Tb == 0) {  // (feasible without frames: an empty label)
    for (int i = tid; i < U; i += ALIGN_THREADS) {
      if (first_out) first_out[i] = -1;
      if (last_out) last_out[i] = -1;
      if (ls_out) ls_out[i] = (OPT && feasible && i < L) ? 0.f : -__builtin_inff();  // (feasible without frames: an empty run)
    }
    return;
  }

  // ---- the back-trace ----
  // Blocks of BF frames, last first: waves 1..4 bring the back-pointer rows of the previous block into LDS while wave 0 walks the
  // current one there (every lane walks the same state: its LDS reads are broadcasts) and writes the block's outputs coalesced.
  Word *const tb = reinterpret_cast<Word *>(smem);
  auto fetch = [&](int blk) {
    const int f0 = blk * BF;
    const int nf = Tb - f0 < BF ? Tb - f0 : BF;
    const uint4 *src = reinterpret_cast<const uint4 *>(bp + (size_t)f0 * 64);  // (rows are 64 * sizeof(Word) bytes: multiples of 64)
    uint4 *dst = reinterpret_cast<uint4 *>(tb + (blk & 1) * BF * 64);
    const int n16 = nf * 64 * (int)sizeof(Word) / 16;
    for (int k = tid - 64; k < n16; k += ALIGN_THREADS - 64) dst[k] = src[k];
  };
  const int nblk = (Tb + BF - 1) / BF;
  int si = OPT ? fin_pos_s : L - 1, sopen = fin_open_s;  // state after the frame being decoded
  int nxt = -1;                        // label index of the frame behind the one being decoded
  if (wave > 0) fetch(nblk - 1);
  __syncthreads();
  for (int blk = nblk - 1; blk >= 0; --blk) {
    if (wave > 0) {
      if (blk > 0) fetch(blk - 1);
    } else {
      const int f0 = blk * BF;
      const int nf = Tb - f0 < BF ? Tb - f0 : BF;
      const Word *const w = tb + (blk & 1) * BF * 64;
      int mytok = -1, myidx = -1;
      unsigned myends = 0;  // bit 0: the frame is the first of its label, bit 1: the last
      for (int fl = nf - 1; fl >= 0; --fl) {
        int tok = blank, idx = -1;
        unsigned ends = 0;
        if (si >= 0) {
          const Word word = w[fl * 64 + si / NL];
          if (KIND == 0) {
            const unsigned c = (unsigned)(word >> (3 * (si & (NL - 1)))) & 7u;
            if (sopen) {
              tok = lab_s[si]; idx = si;
              const unsigned src = c & 3u;
              if (src == 1) { --si; sopen = 0; ends = 1; }
              else if (src == 2) { --si; ends = 1; }
              else if (OPT && src == 3) {  // over an optional wildcard: the spare bit says which state two back
                sopen = (int)((unsigned)(word >> (3 * NL + (si & (NL - 1)))) & 1u);
                si -= 2; ends = 1;
              }
            } else if (c & 4u) {
              sopen = 1;
            }
          } else if (OPT && ((unsigned)(word >> (NL + (si & (NL - 1)))) & 1u)) {  // entered from two back (it outranks bit j)
            tok = lab_s[si]; idx = si;
            si -= 2; ends = 1;
          } else if ((unsigned)(word >> (si & (NL - 1))) & 1u) {
            tok = lab_s[si]; idx = si;
            --si; ends = 1;
          } else if (is_wild(lab_s[si])) {  // a horizontal step behind a wildcard's entry: still the wildcard's
            tok = ALIGN_WILDCARD; idx = si;
          }
          if (OPT && tok == ALIGN_OPTIONAL) tok = ALIGN_WILDCARD;  // (the sentinel of "a_t goes here")
          if (si < 0) sopen = 0;
        }
        if (idx >= 0 && idx != nxt) ends |= 2u;
        nxt = idx;
        if (lane == fl) { mytok = tok; myidx = idx; myends = ends; }
      }
      if (lane < nf) {
        const int t = f0 + lane;
        if (mytok == ALIGN_WILDCARD) mytok = atw[t];
        tok_out[t] = mytok;
        if (idx_out) idx_out[t] = myidx;
        lpw[t] = (double)row_load1(xb + (size_t)((long)t * p.xst) * esz, mytok, dt) - lpw[t];  // (log-probability input: LSE_t = 0)
        if (myends & 1u) first_s[myidx] = t;
        if (myends & 2u) last_s[myidx] = t;
      }
    }
    __syncthreads();
  }

  // ---- per label: first and last frame, and the log-probability of its frames in time order ----
  for (int i = tid; i < U; i += ALIGN_THREADS) {
    int f = -1, l = -1;
    double s = NINF;
    if (i < L) {
      f = first_s[i]; l = last_s[i];
      if (f >= 0) {
        s = 0.0;
        for (int t = f; t <= l; ++t) s += lpw[t];
      } else if (OPT && lab_s[i] == ALIGN_OPTIONAL) {
        s = 0.0;  // skipped: an empty run
      }
    }
    if (first_out) first_out[i] = f;
    if (last_out) last_out[i] = l;
    if (ls_out) ls_out[i] = (float)s;
  }
}

template <int KIND, int NL, bool WIN, bool OPT>
hipError_t launch_align_wild(const Problem &p, char *ws, size_t off_lp, size_t off_at, float *score, int *tokens, int *label_index,
                             int *first_frame, int *last_frame, float *label_score, const int32_t *win, int wstride, hipStream_t st) {
  hipLaunchKernelGGL((align_wild_kernel<KIND, NL, WIN, OPT>), dim3(p.B), dim3(ALIGN_THREADS), 0, st, p, ws, off_lp, off_at, score, tokens,
                     label_index, first_frame, last_frame, label_score, win, wstride);
  return hipGetLastError();
}

}  // namespace

size_t align_wild_workspace_bytes(int B, int T, int U) {
  return r256((size_t)B * T * 64 * bp_word_bytes(nl_for(U))) + r256((size_t)B * T * 8) + r256((size_t)B * T * 4);
}

#define CTC_ALIGN_WILD_ROW(KIND, WIN, OPT)                                                                                       \
  {launch_align_wild<KIND, 1, WIN, OPT>, launch_align_wild<KIND, 2, WIN, OPT>, launch_align_wild<KIND, 4, WIN, OPT>, \
   launch_align_wild<KIND, 8, WIN, OPT>, launch_align_wild<KIND, 16, WIN, OPT>}

hipError_t run_align_wild(const Problem &p, char *ws, float *score, int *tokens, int *label_index, int *first_frame, int *last_frame,
                          float *label_score, hipStream_t st, const int32_t *frame_window, int window_stride, bool optional_wildcards) {
  typedef hipError_t Launch(const Problem &, char *, size_t, size_t, float *, int *, int *, int *, int *, float *, const int32_t *, int,
                            hipStream_t);
  static Launch *const table[3][2][5] = {{CTC_ALIGN_WILD_ROW(0, false, false), CTC_ALIGN_WILD_ROW(1, false, false)},
                                         {CTC_ALIGN_WILD_ROW(0, true, false), CTC_ALIGN_WILD_ROW(1, true, false)},
                                         // (classic, NL = 16 with OPT needs scratch: not built, U <= ALIGN_OPTIONAL_CLASSIC_MAX_U)
                                         {{launch_align_wild<0, 1, false, true>, launch_align_wild<0, 2, false, true>,
                                           launch_align_wild<0, 4, false, true>, launch_align_wild<0, 8, false, true>, nullptr},
                                          CTC_ALIGN_WILD_ROW(1, false, true)}};
  const int NL = nl_for(p.U);
  const int lg = NL == 1 ? 0 : NL == 2 ? 1 : NL == 4 ? 2 : NL == 8 ? 3 : NL == 16 ? 4 : -1;
  if (lg < 0 || p.kind < 0 || p.kind > 1 || (frame_window && optional_wildcards)) return hipErrorInvalidValue;
  const size_t off_lp = r256((size_t)p.B * p.T * 64 * bp_word_bytes(NL));
  const size_t off_at = off_lp + r256((size_t)p.B * p.T * 8);
  Launch *const launch = table[optional_wildcards ? 2 : frame_window ? 1 : 0][p.kind][lg];
  if (!launch) return hipErrorInvalidValue;
  return launch(p, ws, off_lp, off_at, score, tokens, label_index, first_frame, last_frame, label_score,
                                                 frame_window, window_stride, st);
}

}  // namespace ctc
