// Long-form forced alignment of partial transcripts: ctc_amd_long_wildcard_best_path (include/ctc_amd.h), DESIGN.md section 5.19.
//
// The tiled lattice of ctc_align_long.hip (label blocks of UB = 1024 positions x time blocks of TF frames, one launch per
// anti-diagonal of tiles, rows and columns handed over in float64, the blocked back-trace across label blocks) with the wildcard
// positions and the per-label scores of ctc_align_wild.hip.  Both units stay as they are: what is file-local there is repeated here.
// Where the two designs meet:
//   row statistics   the V-wide row pass runs in label block 0 only, as in ctc_align_long.hip, and there it is the one-pass lane
//                    statistic of ctc_align_wild.hip: (m_t, a_t, LSE_t) of every frame go to the workspace.  Tile (k, j), k > 0,
//                    runs on a later launch than tile (0, j) and reads m_t from there.  Every producer puts m_t into the ring
//                    slots of its tile's wildcard positions and beside the blank's emission, so the chain reads emissions as before.
//   block boundary   classic: the `allow` bit of position k * UB looks at label[k * UB - 1], element 0 of the tile's label array,
//                    and is set when either side is a wildcard.  Simplified: the horizontal step of a wildcard position costs
//                    m_t; that is part of the position's own update, in the tile that owns it, so the column (the state of
//                    position k * UB - 1 BEFORE the frame) hands over exactly what the next block's diagonal step needs.
//   skipped tiles    every position, a wildcard too, takes a frame of its own: "position i is -inf before frame i" holds, and
//                    so do the three skip tests.  Block 0 runs for every frame below T_b of an utterance that is not refused by
//                    the count (labels > frames), so a tile further right never reads statistics that were not written.
//   back-trace       the walk of align_long_trace_kernel.  A frame in the open state of a wildcard (classic), or its entry and every
//                    horizontal step behind it (simplified), is the wildcard's: token a_t.  LSE_t becomes lp[t, pi_t] in place.
//   per label        first_frame / last_frame: the frame-parallel scheme of ctc_align_long.hip.  label_score: the thread that sees
//                    a label's first frame is its one writer and sums the label's contiguous frames in time order in float64.
//   windows          WIN (ctc_amd_long_windowed_best_path): every lane holds the (first, last) frames of its
//                    own NL positions of the tile's label block; the producers compare them with the absolute frame and write -inf
//                    outside, a wildcard's m_t included, so the horizontal step behind a wildcard costs its ring slot.  A window
//                    knows nothing of tiles: it acts the same on either side of a time-block or label-block boundary.  The three
//                    skip tests stay true (a window only takes frames away), and nothing behind the ring knows of windows.
// Vector stores only, no atomics, one writer per element: the same bits on every run, and -- score's last bits apart -- for every
// frames_per_tile and batch composition.
#include "ctc_align_long_wild.h"
#include "ctc_align_long.h"
#include "ctc_align_step.h"
#include "ctc_align_wild.h"
#include "ctc_common.h"

namespace ctc {
namespace {

constexpr int NL = LONG_NL, UB = LONG_UB, RW = LONG_ROW_DOUBLES;
constexpr int F = ALIGN_RING / UB;  // frames per ring block
static_assert(F == LONG_RING_FRAMES && F == ALIGN_PW, "one frame per producer wavefront and ring block");
constexpr int RS = UB + 4;          // ring row: UB label emissions, then the blank's, then the row maximum
constexpr int TRACE_BF = 64;        // frames per back-trace block: one per lane of the walking wavefront
constexpr int TRACE_W = 16;         // lanes' words per frame in the window: two blocks of frames move the walk by <= 128 positions = 9 lanes
static_assert(TRACE_W * NL >= 2 * TRACE_BF + 2 * NL, "the window covers the walk of two blocks");
constexpr float FLT_LOWEST = -3.402823466e38f;
constexpr int NO_INDEX = 0x7fffffff;
typedef BpWord<NL>::type Word;
typedef BpBits<NL>::type Bits;

struct LongWildWs {  // device pointers into the workspace (LongWildPlan offsets)
  Word *bp;
  double *col, *row, *lse;
  int *idx, *flag;
  double *mx;  // m_t
  int *arg;    // a_t
  double *lp;  // the sweep: LSE_t; the back-trace: lp[t, pi_t]
};

// Running statistic of one lane (that of ctc_align_wild.hip): m = the maximum so far (-inf before the first element), idx = the
// lowest index holding it, s = sum of exp(x - max(m, FLT_LOWEST)).  A lane visits its indices in ascending order, so a strict
// comparison keeps the lowest one.  with_sum == false (log-probability input; the same in every lane): no sum is needed.
__device__ __forceinline__ void wild_stat_add4(float &m, int &idx, float &s, const float4 v, int k, bool with_sum) {
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

// One frame of the chain: classic, align_chain_step as it stands (a wildcard shows in `allow` and in its emission only); simplified,
// the step of ctc_align_wild.hip: the horizontal step of a wildcard position costs the row maximum emd instead of the blank's ebd.
template <int KIND, bool WIN>
__device__ __forceinline__ Bits wild_chain_step(double (&O)[NL], double (&C)[NL], unsigned allow, unsigned wild, double fillO,
                                                double fillC, const float (&e)[NL], double ebd, double emd) {
  if (KIND == 0) return align_chain_step<0, NL>(O, C, allow, fillO, fillC, e, ebd);
  Bits bits = 0;
  const double pS = from_prev_lane(C[NL - 1], fillC);
#pragma unroll
  for (int j = NL - 1; j >= 0; --j) {
    const double q = j > 0 ? C[j > 0 ? j - 1 : 0] : pS;
    const double dg = q + (double)e[j], h = C[j] + (((wild >> j) & 1u) ? (WIN ? (double)e[j] : emd) : ebd);
    const unsigned sd = dg > h ? 1u : 0u;
    C[j] = sd ? dg : h;
    bits |= (Bits)sd << j;
  }
  return bits;
}

template <int KIND, bool WIN>
__global__ __launch_bounds__(ALIGN_THREADS) void align_long_wild_tile_kernel(const Problem p, const LongWildWs w, int K, int J, int TF,
                                                                             int d, int k_lo, int count,
                                                                             const int32_t *__restrict__ win, int wstride) {
  const double NINF = -__builtin_inf();
  __shared__ __attribute__((aligned(16))) float ring[2 * F * RS];
  __shared__ int lab_s[UB + 1];  // validated labels (-1: no emission, ALIGN_WILDCARD: a wildcard) of positions k * UB - 1 .. k * UB + UB - 1
  __shared__ double col_s[2][F][2];
  __shared__ double lse_s[ALIGN_PW];

  const int b = blockIdx.x / count, k = k_lo + blockIdx.x % count, j = d - k;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = p.T, V = p.V, blank = p.blank, dt = p.xdtype;
  const int Tb = frame_count(p, b);
  const int L = label_count(p, b);
  const int t_lo = j * TF;                                   // (J * TF < T + TF: no overflow)
  const int t_hi = Tb - t_lo < TF ? Tb : t_lo + TF;          // one past the tile's last frame
  if (too_many_labels(p, L) || L > Tb) return;               // infeasible by the count (every position takes a frame): the trace says so
  if (t_lo >= Tb || (k > 0 && k * UB >= L)) return;          // beyond the frames / beyond the labels
  if (t_lo + TF - 1 < k * UB) return;                        // position i is -inf before frame i
  const bool fresh = t_lo <= k * UB;                         // ... so this is the block's first tile (j == 0 included)
  const bool has_right = k + 1 < K && (k + 1) * UB < L;

  for (int i = tid; i <= UB; i += ALIGN_THREADS) {
    const int g = k * UB + i - 1;
    int tok = -1;
    if (g >= 0 && g < L) tok = label_at(p, label_row(p, b), g);
    lab_s[i] = tok == ALIGN_WILDCARD ? ALIGN_WILDCARD : emits(p, tok) ? tok : -1;
  }
  __syncthreads();

  int lab[NL];
  unsigned wild = 0;  // bit q = position k * UB + lane * NL + q is a wildcard
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    lab[q] = lab_s[1 + lane * NL + q];
    if (lab[q] == ALIGN_WILDCARD) wild |= 1u << q;
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
  const bool with_sum = p.wrt == 0;
  Word *const bp = w.bp + ((size_t)b * K + k) * (size_t)T * 64;
  double *const row = w.row + ((size_t)b * K + k) * RW;
  const double *const col_in = k > 0 ? w.col + ((size_t)b * (K - 1) + (k - 1)) * (size_t)T * 2 : nullptr;
  double *const col_out = has_right ? w.col + ((size_t)b * (K - 1) + k) * (size_t)T * 2 : nullptr;
  double *const mxw = w.mx + (size_t)b * T;
  int *const argw = w.arg + (size_t)b * T;
  double *const lpw = w.lp + (size_t)b * T;

  // chain state (wave 0): row in
  double O[NL], C[NL];  // simplified: C is S, O unused
  unsigned allow = 0;   // classic: bit q = label[i] differs from label[i-1], or one of the two is a wildcard
  double cs = 0.0;      // the start state (label block 0): blank so far
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    O[q] = NINF; C[q] = NINF;
    const int i = lane * NL + q;
    if (KIND == 0 && k * UB + i > 0) {
      const int prev = lab_s[i];
      if (lab[q] != prev || lab[q] == ALIGN_WILDCARD || prev == ALIGN_WILDCARD) allow |= 1u << q;
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
    if (k == 0) {
      // the row pass.  Both access paths give a lane the same elements in the same order -- k .. k+3 for k = 4 * lane, + 256, ... --
      // so their results are the same bits (an element past V enters as -inf: it never wins and adds exp(-inf) = 0)
      float m = -__builtin_inff(), s = 0.f;
      int ix = lane * 4 < V ? lane * 4 : NO_INDEX;
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
        wild_stat_add4(m, ix, s, v, c, with_sum);
      }
      M = wave_max(m);
      // every lane whose maximum is the row's offers its lowest index; an all -inf row: every lane does, index 0 wins
      unsigned a = wave_min_u(m == M ? (unsigned)ix : (unsigned)NO_INDEX);
      if (a >= (unsigned)V) a = 0;  // (NaN rows only: unspecified, but a token of the vocabulary)
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
      }
    } else {
      M = (float)mxw[t];  // (tile (0, j) stored it on an earlier launch; a float32 value, so the round trip is exact)
    }
    float *const r = ring + ((kb & 1) * F + f) * RS;
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      float v = ((wild >> q) & 1u) ? M : e[q];
      if constexpr (WIN) {
        if (t < wf[q] || t > wl[q]) v = -__builtin_inff();
      }
      r[lane * NL + q] = v;
    }
    if (lane == 0) { r[UB] = eb; r[UB + 1] = M; }
    if (k > 0 && lane < 2) col_s[kb & 1][f][lane] = col_in[(size_t)t * 2 + lane];
  };

  auto consume = [&](int kb) {
    const int t0 = t_lo + kb * F;
    const int nf = t_hi - t0 < F ? t_hi - t0 : F;
    const float *const rb = ring + (kb & 1) * F * RS;
    float e[NL], en[NL], eb, ebn, em = 0.f, emn = 0.f;
#pragma unroll
    for (int q = 0; q < NL; ++q) en[q] = rb[lane * NL + q];
    ebn = rb[UB];
    if (KIND == 1) emn = rb[UB + 1];
    for (int f = 0; f < nf; ++f) {
#pragma unroll
      for (int q = 0; q < NL; ++q) e[q] = en[q];
      eb = ebn; em = emn;
      {  // the next frame's emissions, one frame ahead of their use (past the block: the last row again)
        const float *const rn = rb + (f + 1 < F ? f + 1 : F - 1) * RS;
#pragma unroll
        for (int q = 0; q < NL; ++q) en[q] = rn[lane * NL + q];
        ebn = rn[UB];
        if (KIND == 1) emn = rn[UB + 1];
      }
      const double ebd = (double)eb;
      if (col_out && lane == 63) {  // column out: the last position before this frame
        col_out[(size_t)(t0 + f) * 2] = O[NL - 1];
        col_out[(size_t)(t0 + f) * 2 + 1] = C[NL - 1];
      }
      const double fillO = k > 0 ? col_s[kb & 1][f][0] : NINF;
      const double fillC = k > 0 ? col_s[kb & 1][f][1] : cs;
      const Bits bits = wild_chain_step<KIND, WIN>(O, C, allow, wild, fillO, fillC, e, ebd, (double)em);
      cs += ebd;
      bp[(size_t)(t0 + f) * 64 + lane] = (Word)bits;
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

template <int KIND>
__global__ __launch_bounds__(ALIGN_THREADS) void align_long_wild_trace_kernel(const Problem p, const LongWildWs w, int K, int J, int TF,
                                                                              float *__restrict__ score, int *__restrict__ tokens,
                                                                              int *__restrict__ label_index) {
  const double NINF = -__builtin_inf();
  __shared__ __attribute__((aligned(16))) Word tb[2 * TRACE_BF * TRACE_W];
  __shared__ double lsum_s[64];
  __shared__ double fin_s;
  __shared__ int fin_open_s, si_s;

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = p.T, blank = p.blank, dt = p.xdtype;
  const int Tb = frame_count(p, b);
  const int L = label_count(p, b);
  const int32_t *const lrow = label_row(p, b);

  // ---- the end state ----
  if (wave == 0) {
    const int nj = (Tb + TF - 1) / TF;
    double s = 0.0;
    if (p.wrt == 0)
      for (int j = lane; j < nj; j += 64) s += w.lse[(size_t)b * J + j];
    lsum_s[lane] = s;
  } else if (tid == 64) {
    double best = NINF;
    int open = 0;
    if (too_many_labels(p, L) || L > Tb) {
    } else if (Tb == 0) {
      best = 0.0;  // no frames, no labels
    } else if (L == 0) {
      best = w.row[(size_t)b * K * RW + 2 * UB];
    } else {
      const int i = L - 1, r = i % UB;
      const double *const row = w.row + ((size_t)b * K + i / UB) * RW;
      const double ov = row[(r % NL) * 64 + r / NL], cv = row[(NL + r % NL) * 64 + r / NL];
      const bool op = KIND == 0 && ov > cv;
      best = op ? ov : cv;
      open = op ? 1 : 0;
    }
    fin_s = best;
    fin_open_s = open;
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
  // Blocks of TRACE_BF frames, last first.  The walk loses at most one position per frame, so from the position at which a block
  // starts the words of the TRACE_W lanes at and below it cover that block and the one before: waves 1..4 fetch that window of the
  // previous block while wave 0 walks the current one in LDS (every lane walks the same state) and writes its outputs coalesced.
  // The walk notes a position per frame and, simplified, whether the frame is a horizontal step behind it: whether that position
  // is a wildcard is looked up after the block, one lane per frame, off the walk's dependency chain.
  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  const int *const argw = w.arg + (size_t)b * T;
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
  int si = L - 1, sopen = fin_open_s;  // state after the frame being decoded
  int g_cur = window(si);              // window of the block being walked
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
      int mypos = -1, myhoriz = 0;
      for (int fl = nf - 1; fl >= 0; --fl) {
        int pos = -1, horiz = 0;
        if (si >= 0) {
          const Word word = wd[fl * TRACE_W + (si / NL - g_cur)];
          if (KIND == 0) {
            const unsigned c = (unsigned)(word >> (3 * (si & (NL - 1)))) & 7u;
            if (sopen) {
              pos = si;
              const unsigned src = c & 3u;
              if (src == 1) { --si; sopen = 0; }
              else if (src == 2) --si;
            } else if (c & 4u) {
              sopen = 1;
            }
          } else if ((unsigned)(word >> (si & (NL - 1))) & 1u) {
            pos = si;
            --si;
          } else {  // a horizontal step behind position si: the wildcard's frame if si is one, a blank otherwise
            pos = si;
            horiz = 1;
          }
          if (si < 0) sopen = 0;
        }
        if (lane == fl) { mypos = pos; myhoriz = horiz; }
      }
      if (lane < nf) {
        const int t = f0 + lane;
        int tok = blank, idx = -1;
        if (mypos >= 0) {
          const int lt = label_at(p, lrow, mypos);
          if (lt == ALIGN_WILDCARD) { tok = argw[t]; idx = mypos; }
          else if (!myhoriz) { tok = lt; idx = mypos; }
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

// first_frame / last_frame from label_index: thread n looks at frame n (a label's first frame is the one whose predecessor shows
// another index, its last the one whose successor does: one writer per element) and at label position n (-1 from label_length on
// and for an infeasible utterance)
__global__ __launch_bounds__(256) void align_long_wild_frames_kernel(const Problem p, const int *__restrict__ idx,
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

// label_score from label_index and lp[t, pi_t]: thread n looks at frame n; where it is the first frame of label i the thread is
// that label's one writer and adds up the label's frames -- contiguous on both lattices -- in time order in float64, eight loads
// in flight at a time (a wildcard may own tens of thousands of frames).  ... and at label position n: -inf from label_length on
// and for an infeasible utterance (every label of a feasible one owns a frame).
__global__ __launch_bounds__(256) void align_long_wild_score_kernel(const Problem p, const int *__restrict__ idx,
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

}  // namespace

hipError_t run_align_long_wild(const Problem &p, const LongWildPlan &W, char *ws, float *score, int *tokens, int *label_index,
                               int *first_frame, int *last_frame, float *label_score, hipStream_t st, const int32_t *frame_window,
                               int window_stride) {
  if (p.kind < 0 || p.kind > 1) return hipErrorInvalidValue;
  const LongPlan &P = W.base;
  LongWildWs w;
  w.bp = reinterpret_cast<Word *>(ws + P.off_bp);
  w.col = reinterpret_cast<double *>(ws + P.off_col);
  w.row = reinterpret_cast<double *>(ws + P.off_row);
  w.lse = reinterpret_cast<double *>(ws + P.off_lse);
  w.idx = reinterpret_cast<int *>(ws + P.off_idx);
  w.flag = reinterpret_cast<int *>(ws + P.off_flag);
  w.mx = reinterpret_cast<double *>(ws + W.off_max);
  w.arg = reinterpret_cast<int *>(ws + W.off_arg);
  w.lp = reinterpret_cast<double *>(ws + W.off_lp);
  if (p.T > 0) {
    for (int d = 0; d < P.launches; ++d) {
      int k_lo, count;
      long_diagonal(P, d, &k_lo, &count);
      const dim3 grid((unsigned)((size_t)p.B * count));
      const auto tile = frame_window ? (p.kind == 0 ? align_long_wild_tile_kernel<0, true> : align_long_wild_tile_kernel<1, true>)
                                     : (p.kind == 0 ? align_long_wild_tile_kernel<0, false> : align_long_wild_tile_kernel<1, false>);
      hipLaunchKernelGGL(tile, grid, dim3(ALIGN_THREADS), 0, st, p, w, P.K, P.J, P.TF, d, k_lo, count, frame_window, window_stride);
    }
  }
  if (p.kind == 0) hipLaunchKernelGGL(align_long_wild_trace_kernel<0>, dim3(p.B), dim3(ALIGN_THREADS), 0, st, p, w, P.K, P.J, P.TF, score, tokens, label_index);
  else hipLaunchKernelGGL(align_long_wild_trace_kernel<1>, dim3(p.B), dim3(ALIGN_THREADS), 0, st, p, w, P.K, P.J, P.TF, score, tokens, label_index);
  const int per_b = ((p.T > p.U ? p.T : p.U) + 255) / 256;
  const int *const idx = label_index ? label_index : w.idx;
  if ((first_frame || last_frame) && per_b > 0)
    hipLaunchKernelGGL(align_long_wild_frames_kernel, dim3((unsigned)((size_t)p.B * per_b)), dim3(256), 0, st, p, idx, w.flag, per_b,
                       first_frame, last_frame);
  if (label_score && per_b > 0)
    hipLaunchKernelGGL(align_long_wild_score_kernel, dim3((unsigned)((size_t)p.B * per_b)), dim3(256), 0, st, p, idx, w.flag, w.lp,
                       per_b, label_score);
  return hipGetLastError();
}

}  // namespace ctc
