// Long-form best-path (Viterbi) forced alignment: ctc_amd_long_best_path (include/ctc_amd.h), DESIGN.md section 5.18.
//
// The lattice of ctc_align.hip, tiled over label blocks x time blocks so that the label axis of one long recording spreads over
// many workgroups.  Tile (k, j) covers label positions k * UB .. k * UB + UB - 1 (UB = 1024: 16 per lane, the chain step of
// align_kernel<KIND, 16>, ctc_align_step.h) and frames j * TF .. j * TF + TF - 1.  Launch d runs every tile with k + j = d: a tile
// needs its left neighbour (k - 1, j) and its predecessor in time (k, j - 1), both on diagonal d - 1, so the order of the launches
// on the stream is the only dependency.  No workgroup waits for another; no flags, no cooperative launch, no atomics.
//
// One workgroup per (utterance, tile), the roles of ctc_align.hip: wave 0 is the chain, waves 1..4 gather x[t, label[i]] and
// x[t, blank] into the LDS ring one block of 4 frames ahead.  What a tile adds:
//   row     the chain state (O, C per position, float64; block 0: also the start state) comes from the (utterance, label block)
//           row buffer and goes back there.  A tile before which no frame could have reached the block starts from -inf;
//   column  lane 0's fill is the state of position k * UB - 1 BEFORE frame t, which tile (k - 1, j) stored per frame on the
//           previous launch; the producers stage it through LDS with the ring block.  A tile with a label block to its right
//           stores that pair for its last position;
//   LSE     the V-wide row pass runs in label block 0 only; its float64 sum per (utterance, time block) is added up by the trace.
// Tiles no path passes are skipped: time blocks beyond logit_length, label blocks beyond label_length, blocks whose first position
// needs more frames than have gone by, and every tile of an utterance with more labels than frames (the trace reports it).
// An active tile's neighbours on diagonal d - 1 are active or of the "-inf start" kind, so nothing unwritten is ever read.  (Tiles
// from which the end cannot be reached any more are NOT skipped: their columns would have to read as -inf one frame late.)
//
// Then one trace workgroup per utterance: end state from the rows, LSE partials in a fixed order, walk back across tiles with a
// window of 16 lanes' back-pointer words per frame fetched into LDS one block of 64 frames ahead; and, on request, a frame-parallel
// kernel that derives first_frame / last_frame from label_index (each element has exactly one writer).
// float64 max and add hand over exactly, so the path does not depend on TF or B; `score` may differ in its last bits between
// tilings (the order of the LSE sum).
#include "ctc_align_long.h"
#include "ctc_align_step.h"
#include "ctc_common.h"

namespace ctc {
namespace {

constexpr int NL = LONG_NL, UB = LONG_UB, RW = LONG_ROW_DOUBLES;
constexpr int F = ALIGN_RING / UB;  // frames per ring block
static_assert(F == LONG_RING_FRAMES && F == ALIGN_PW, "one frame per producer wavefront and ring block");
constexpr int RS = UB + 4;          // ring row: UB label emissions, then the blank's
constexpr int TRACE_BF = 64;        // frames per back-trace block: one per lane of the walking wavefront
constexpr int TRACE_W = 16;         // lanes' words per frame in the window: two blocks of frames move the walk by <= 128 positions = 9 lanes
static_assert(TRACE_W * NL >= 2 * TRACE_BF + 2 * NL, "the window covers the walk of two blocks");
typedef BpWord<NL>::type Word;
typedef BpBits<NL>::type Bits;

struct LongWs {  // device pointers into the workspace (LongPlan offsets)
  Word *bp;
  double *col, *row, *lse;
  int *idx, *flag;
};

template <int KIND>
__global__ __launch_bounds__(ALIGN_THREADS) void align_long_tile_kernel(const Problem p, const LongWs w, int K, int J, int TF, int d,
                                                                        int k_lo, int count) {
  const double NINF = -__builtin_inf();
  __shared__ __attribute__((aligned(16))) float ring[2 * F * RS];
  __shared__ int lab_s[UB + 1];  // validated labels (-1: no emission) of positions k * UB - 1 .. k * UB + UB - 1
  __shared__ double col_s[2][F][2];
  __shared__ double lse_s[ALIGN_PW];

  const int b = blockIdx.x / count, k = k_lo + blockIdx.x % count, j = d - k;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = p.T, V = p.V, dt = p.xdtype;
  const int Tb = frame_count(p, b);
  const int L = label_count(p, b);
  const int t_lo = j * TF;                                   // (J * TF < T + TF: no overflow)
  const int t_hi = Tb - t_lo < TF ? Tb : t_lo + TF;          // one past the tile's last frame
  if (too_many_labels(p, L) || L > Tb) return;               // infeasible: the trace says so
  if (t_lo >= Tb || (k > 0 && k * UB >= L)) return;          // beyond the frames / beyond the labels
  if (t_lo + TF - 1 < k * UB) return;                        // position i is -inf before frame i
  const bool fresh = t_lo <= k * UB;                         // ... so this is the block's first tile (j == 0 included)
  const bool has_right = k + 1 < K && (k + 1) * UB < L;

  for (int i = tid; i <= UB; i += ALIGN_THREADS) {
    const int g = k * UB + i - 1;
    int tok = -1;
    if (g >= 0 && g < L) tok = label_at(p, label_row(p, b), g);
    lab_s[i] = emits(p, tok) ? tok : -1;
  }
  __syncthreads();

  int lab[NL];
#pragma unroll
  for (int q = 0; q < NL; ++q) lab[q] = lab_s[1 + lane * NL + q];

  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  const bool vec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (dt == 0 ? 15 : 7)) == 0;
  const bool stats = k == 0 && p.wrt == 0;
  Word *const bp = w.bp + ((size_t)b * K + k) * (size_t)T * 64;
  double *const row = w.row + ((size_t)b * K + k) * RW;
  const double *const col_in = k > 0 ? w.col + ((size_t)b * (K - 1) + (k - 1)) * (size_t)T * 2 : nullptr;
  double *const col_out = has_right ? w.col + ((size_t)b * (K - 1) + k) * (size_t)T * 2 : nullptr;

  // chain state (wave 0): row in
  double O[NL], C[NL];  // simplified: C is S, O unused
  unsigned allow = 0;   // classic: bit q = label[i] differs from label[i-1]
  double cs = 0.0;      // the start state (label block 0): blank so far
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    O[q] = NINF; C[q] = NINF;
    const int i = lane * NL + q;
    if (KIND == 0 && k * UB + i > 0 && lab[q] != lab_s[i]) allow |= 1u << q;
  }
  if (wave == 0 && !fresh) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      if (KIND == 0) O[q] = row[q * 64 + lane];
      C[q] = row[(NL + q) * 64 + lane];
    }
    if (k == 0) cs = row[2 * UB];
  }
  double lse = 0.0;  // producers: sum of the LSE of this wavefront's frames

  auto produce = [&](int kb) {  // one frame per producer wavefront
    const int f = wave - 1, t = t_lo + kb * F + f;
    if (t >= t_hi) return;
    align_produce<NL, 1>(p, xb, esz, vec, lab, t, t_hi, ring + ((kb & 1) * F + f) * RS, lane, stats, lse);
    if (k > 0 && lane < 2) col_s[kb & 1][f][lane] = col_in[(size_t)t * 2 + lane];
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
      if (col_out && lane == 63) {  // column out: the last position before this frame
        col_out[(size_t)(t0 + f) * 2] = O[NL - 1];
        col_out[(size_t)(t0 + f) * 2 + 1] = C[NL - 1];
      }
      const double fillO = k > 0 ? col_s[kb & 1][f][0] : NINF;
      const double fillC = k > 0 ? col_s[kb & 1][f][1] : cs;
      const Bits bits = align_chain_step<KIND, NL>(O, C, allow, fillO, fillC, e, ebd);
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
__global__ __launch_bounds__(ALIGN_THREADS) void align_long_trace_kernel(const Problem p, const LongWs w, int K, int J, int TF,
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
  const int T = p.T, blank = p.blank;
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
      int myidx = -1;
      for (int fl = nf - 1; fl >= 0; --fl) {
        int idx = -1;
        if (si >= 0) {
          const Word word = wd[fl * TRACE_W + (si / NL - g_cur)];
          if (KIND == 0) {
            const unsigned c = (unsigned)(word >> (3 * (si & (NL - 1)))) & 7u;
            if (sopen) {
              idx = si;
              const unsigned src = c & 3u;
              if (src == 1) { --si; sopen = 0; }
              else if (src == 2) --si;
            } else if (c & 4u) {
              sopen = 1;
            }
          } else if ((unsigned)(word >> (si & (NL - 1))) & 1u) {
            idx = si;
            --si;
          }
          if (si < 0) sopen = 0;
        }
        if (lane == fl) myidx = idx;
      }
      if (lane < nf) {
        tok_out[f0 + lane] = myidx >= 0 ? label_at(p, lrow, myidx) : blank;
        idx_out[f0 + lane] = myidx;
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
__global__ __launch_bounds__(256) void align_long_frames_kernel(const Problem p, const int *__restrict__ idx, const int *__restrict__ flag,
                                                                int per_b, int *__restrict__ first_frame, int *__restrict__ last_frame) {
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

}  // namespace

hipError_t run_align_long(const Problem &p, const LongPlan &P, char *ws, float *score, int *tokens, int *label_index, int *first_frame,
                          int *last_frame, hipStream_t st) {
  if (p.kind < 0 || p.kind > 1) return hipErrorInvalidValue;
  LongWs w;
  w.bp = reinterpret_cast<Word *>(ws + P.off_bp);
  w.col = reinterpret_cast<double *>(ws + P.off_col);
  w.row = reinterpret_cast<double *>(ws + P.off_row);
  w.lse = reinterpret_cast<double *>(ws + P.off_lse);
  w.idx = reinterpret_cast<int *>(ws + P.off_idx);
  w.flag = reinterpret_cast<int *>(ws + P.off_flag);
  if (p.T > 0) {
    for (int d = 0; d < P.launches; ++d) {
      int k_lo, count;
      long_diagonal(P, d, &k_lo, &count);
      const dim3 grid((unsigned)((size_t)p.B * count));
      if (p.kind == 0) hipLaunchKernelGGL(align_long_tile_kernel<0>, grid, dim3(ALIGN_THREADS), 0, st, p, w, P.K, P.J, P.TF, d, k_lo, count);
      else hipLaunchKernelGGL(align_long_tile_kernel<1>, grid, dim3(ALIGN_THREADS), 0, st, p, w, P.K, P.J, P.TF, d, k_lo, count);
    }
  }
  if (p.kind == 0) hipLaunchKernelGGL(align_long_trace_kernel<0>, dim3(p.B), dim3(ALIGN_THREADS), 0, st, p, w, P.K, P.J, P.TF, score, tokens, label_index);
  else hipLaunchKernelGGL(align_long_trace_kernel<1>, dim3(p.B), dim3(ALIGN_THREADS), 0, st, p, w, P.K, P.J, P.TF, score, tokens, label_index);
  const int per_b = ((p.T > p.U ? p.T : p.U) + 255) / 256;
  if ((first_frame || last_frame) && per_b > 0)
    hipLaunchKernelGGL(align_long_frames_kernel, dim3((unsigned)((size_t)p.B * per_b)), dim3(256), 0, st, p,
                       label_index ? label_index : w.idx, w.flag, per_b, first_frame, last_frame);
  return hipGetLastError();
}

}  // namespace ctc
