// Best-path (Viterbi) forced alignment for both CTC lattices: ctc_amd_best_path (include/ctc_amd.h), DESIGN.md section 5.6.
//
// The lattice of the loss in the (max, +) semiring, with back-pointers and a back-trace.  The value of a path is
//   sum_t lp[t, pi_t] = sum_t x[t, pi_t] - sum_t LSE_t,
// and the second sum is the same for every path: the recursion runs on the RAW logits with a float64 state (sums of float32
// inputs are exact there, so the chosen path is the exact optimum up to genuine float64 ties), sum_t LSE_t is accumulated on
// the side in float64 from float32 row statistics and subtracted once at the end.  No transcendental on the chain.
//
// One workgroup per utterance, five wavefronts:
//   wave 0      the chain: NL label positions per lane (position i = lane * NL + j), neighbour exchange with DPP, one
//               back-pointer word per lane and frame, stored coalesced (64 * sizeof(word) bytes per frame);
//   waves 1..4  producers: stream the frame's row (float32 / bfloat16 / float16, run-time switch) for its max and sum, gather
//               x[t, blank] and x[t, label[i]] from global memory (the row is in flight or L2-resident then) into an LDS
//               ring one block of frames ahead of the chain.  No V-wide row is staged in LDS: any V costs no LDS.
// Impossible states are -inf (float64 max and add propagate it; nothing on the chain subtracts), so a label outside [0, V) or
// equal to the blank, too few frames and -inf log-probabilities all end in a final value of -inf: the utterance is infeasible.
//
// States.  Classic: O[i] = the last frame emitted label i (open), C[i] = labels 0..i are done and the last frame was blank
// (closed), plus the start state (blank so far), which every lane carries as the running sum `cs` and lane 0 feeds into
// position 0.  Simplified: S[i] = labels 0..i are emitted.
//   O'[i] = max(O[i], C[i-1], O[i-1] if label[i] != label[i-1]) + x[label[i]]      2 bits: 0, 1, 2
//   C'[i] = max(C[i], O[i]) + x[blank]                                            1 bit
//   S'[i] = max(S[i] + x[blank], S[i-1] + x[label[i]])                            1 bit (1 = the frame emits label i)
// Ties keep the first candidate in the order written (strict comparisons): deterministic.
#include "ctc_align_step.h"
#include "ctc_common.h"
#include "ctc_launch.h"

namespace ctc {
namespace {

// frames per back-trace block: two blocks of (frames x 64 lanes x word) fit the LDS the ring used (32 KB)
constexpr int trace_frames(int NL) { return NL == 16 ? 32 : 64; }

template <int KIND, int NL>
__global__ __launch_bounds__(ALIGN_THREADS) void align_kernel(const Problem p, char *__restrict__ ws, float *__restrict__ score,
                                                              int *__restrict__ tokens, int *__restrict__ label_index) {
  typedef typename BpWord<NL>::type Word;
  typedef typename BpBits<NL>::type Bits;
  constexpr int UP = 64 * NL;
  constexpr int F = ALIGN_RING / UP;                 // frames per ring buffer: 64, 32, 16, 8, 4
  constexpr int RS = UP + 4;                         // ring row: UP label emissions, then the blank's
  constexpr int FPW = F / ALIGN_PW;                  // frames per producer wavefront and block
  constexpr int G = FPW < 4 ? FPW : 4;               // ... of which G are in flight together
  constexpr int BF = trace_frames(NL);
  constexpr int RING_BYTES = 2 * F * RS * 4, TRACE_BYTES = 2 * BF * 64 * (int)sizeof(Word);
  constexpr int SMEM = RING_BYTES > TRACE_BYTES ? RING_BYTES : TRACE_BYTES;
  const double NINF = -__builtin_inf();

  __shared__ __attribute__((aligned(16))) char smem[SMEM];  // the ring during the sweep, back-pointer blocks during the back-trace
  __shared__ int lab_s[UP];                                  // validated labels (-1: no emission)
  __shared__ double lse_s[ALIGN_PW];
  __shared__ double fin_s;
  __shared__ int fin_open_s;
  float *const ring = reinterpret_cast<float *>(smem);

  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = p.T, V = p.V, blank = p.blank, dt = p.xdtype;
  const int Tb = frame_count(p, b);
  int L = label_count(p, b);
  const bool too_long = too_many_labels(p, L);
  if (too_long) L = 0;  // (nothing of such an utterance is read; it is reported infeasible below)

  for (int i = tid; i < UP; i += ALIGN_THREADS) {
    int tok = -1;
    if (i < L) tok = label_at(p, label_row(p, b), i);
    lab_s[i] = emits(p, tok) ? tok : -1;
  }
  __syncthreads();

  int lab[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) lab[j] = lab_s[lane * NL + j];

  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  // vector row accesses (16 bytes of float32, 8 bytes of 16-bit elements) need aligned rows; element-wise otherwise
  const bool vec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (dt == 0 ? 15 : 7)) == 0;
  Word *const bp = reinterpret_cast<Word *>(ws) + (size_t)b * T * 64;

  // ---- the sweep ----
  // chain state (wave 0)
  double O[NL], C[NL];  // simplified: C is S, O unused
  unsigned allow = 0;   // classic: bit j = label[i] differs from label[i-1]
  double cs = 0.0;      // the start state: blank so far
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    O[j] = NINF; C[j] = NINF;
    const int i = lane * NL + j;
    if (KIND == 0 && i > 0 && lab[j] != lab_s[i - 1]) allow |= 1u << j;
  }
  double lse = 0.0;  // producers: sum of the LSE of this wavefront's frames

  auto produce = [&](int kb) {
    const int pw = wave - 1, t0 = kb * F;
    float *const rb = ring + (kb & 1) * F * RS;
    for (int f0 = pw * FPW; f0 < (pw + 1) * FPW; f0 += G) {
      if (t0 + f0 >= Tb) break;
      align_produce<NL, G>(p, xb, esz, vec, lab, t0 + f0, Tb, rb + f0 * RS, lane, p.wrt == 0, lse);
    }
  };

  auto consume = [&](int kb) {
    const int t0 = kb * F;
    const int nf = Tb - t0 < F ? Tb - t0 : F;
    const float *const rb = ring + (kb & 1) * F * RS;
    float e[NL], en[NL], eb, ebn;
#pragma unroll
    for (int j = 0; j < NL; ++j) en[j] = rb[lane * NL + j];
    ebn = rb[UP];
    for (int f = 0; f < nf; ++f) {
#pragma unroll
      for (int j = 0; j < NL; ++j) e[j] = en[j];
      eb = ebn;
      {  // the next frame's emissions, one frame ahead of their use (past the block: the last row again)
        const float *const rn = rb + (f + 1 < F ? f + 1 : F - 1) * RS;
#pragma unroll
        for (int j = 0; j < NL; ++j) en[j] = rn[lane * NL + j];
        ebn = rn[UP];
      }
      const double ebd = (double)eb;
      const Bits bits = align_chain_step<KIND, NL>(O, C, allow, NINF, cs, e, ebd);
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
      if (lane == 0) { fin_s = cs; fin_open_s = 0; }
    } else if (lane == i / NL) {
      const bool op = KIND == 0 && ov > cv;
      fin_s = op ? ov : cv;
      fin_open_s = op ? 1 : 0;
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
  for (int t = (feasible ? Tb : 0) + tid; t < T; t += ALIGN_THREADS) {
    tok_out[t] = -1;
    if (idx_out) idx_out[t] = -1;
  }
  if (!feasible || Tb == 0) return;

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
  int si = L - 1, sopen = fin_open_s;  // state after the frame being decoded
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
      for (int fl = nf - 1; fl >= 0; --fl) {
        int tok = blank, idx = -1;
        if (si >= 0) {
          const Word word = w[fl * 64 + si / NL];
          if (KIND == 0) {
            const unsigned c = (unsigned)(word >> (3 * (si & (NL - 1)))) & 7u;
            if (sopen) {
              tok = lab_s[si]; idx = si;
              const unsigned src = c & 3u;
              if (src == 1) { --si; sopen = 0; }
              else if (src == 2) --si;
            } else if (c & 4u) {
              sopen = 1;
            }
          } else if ((unsigned)(word >> (si & (NL - 1))) & 1u) {
            tok = lab_s[si]; idx = si;
            --si;
          }
          if (si < 0) sopen = 0;
        }
        if (lane == fl) { mytok = tok; myidx = idx; }
      }
      if (lane < nf) {
        tok_out[f0 + lane] = mytok;
        if (idx_out) idx_out[f0 + lane] = myidx;
      }
    }
    __syncthreads();
  }
}

template <int KIND, int NL>
hipError_t launch_align(const Problem &p, char *ws, float *score, int *tokens, int *label_index, hipStream_t st) {
  hipLaunchKernelGGL((align_kernel<KIND, NL>), dim3(p.B), dim3(ALIGN_THREADS), 0, st, p, ws, score, tokens, label_index);
  return hipGetLastError();
}

}  // namespace

size_t align_workspace_bytes(int B, int T, int U) {
  return ((size_t)B * T * 64 * bp_word_bytes(nl_for(U)) + 255) & ~size_t(255);
}

hipError_t run_align(const Problem &p, char *ws, float *score, int *tokens, int *label_index, hipStream_t st) {
  typedef hipError_t Launch(const Problem &, char *, float *, int *, int *, hipStream_t);
  static Launch *const table[2][5] = {
      {launch_align<0, 1>, launch_align<0, 2>, launch_align<0, 4>, launch_align<0, 8>, launch_align<0, 16>},
      {launch_align<1, 1>, launch_align<1, 2>, launch_align<1, 4>, launch_align<1, 8>, launch_align<1, 16>}};
  const int NL = nl_for(p.U);
  const int lg = NL == 1 ? 0 : NL == 2 ? 1 : NL == 4 ? 2 : NL == 8 ? 3 : NL == 16 ? 4 : -1;
  if (lg < 0 || p.kind < 0 || p.kind > 1) return hipErrorInvalidValue;
  return table[p.kind][lg](p, ws, score, tokens, label_index, st);
}

}  // namespace ctc
