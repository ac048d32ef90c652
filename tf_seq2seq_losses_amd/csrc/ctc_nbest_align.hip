// N-best forced alignment: the best path of N label sequences per utterance: ctc_amd_nbest_best_path (include/ctc_amd.h), DESIGN.md section 5.12.
//
// The work decomposition of ctc_nbest.hip with the chain and the back-trace of ctc_align.hip.  One workgroup per utterance and
// group of NBEST_G = 8 hypotheses, twelve wavefronts:
//   waves 0..7   the chains: wave g runs the (max, +) recursion of hypothesis n = blockIdx.y * 8 + g on the RAW logits with a
//                float64 state, NL label positions per lane (position i = lane * NL + j), neighbour exchange with DPP, one packed
//                back-pointer word per lane and frame, stored coalesced (64 * sizeof(word) bytes per frame and hypothesis);
//   waves 8..11  producers: stream the frame's row ONCE per group (float32 / bfloat16 / float16, run-time switch) for its max and
//                sum, and gather x[t, blank] and x[t, label[n][i]] of all eight hypotheses into an LDS ring one block of frames
//                ahead of the chains.  No V-wide row is staged in LDS: any V costs no LDS.
// States, candidate order and back-pointer bits are those of ctc_align.hip (strict comparisons, the first candidate wins a tie):
//   O'[i] = max(O[i], C[i-1], O[i-1] if label[i] != label[i-1]) + x[label[i]]      2 bits: 0, 1, 2
//   C'[i] = max(C[i], O[i]) + x[blank]                                            1 bit
//   S'[i] = max(S[i] + x[blank], S[i-1] + x[label[i]])                            1 bit (1 = the frame emits label i)
// Impossible states are -inf.  sum_t LSE_t is accumulated by every chain in frame order from the float32 row statistics the
// producers leave beside the ring (float64 adds) and subtracted once at the end: the same bits for every group and position.
//
// The back-trace: after the sweep the ring's 64 KB become eight double-buffered walk buffers of 2 x 4 KB.  Blocks of BF frames,
// last first: the producers bring the back-pointer rows of the previous block of all eight hypotheses into LDS while every chain
// wavefront walks the current block of its own hypothesis there (every lane walks the same state: its LDS reads are broadcasts).
// Lane fl keeps the label index of frame f0 + fl; after the block the wavefront writes tokens and label_index coalesced, and the
// lane whose label index differs from that of frame f - 1 / f + 1 (DPP neighbours; across block edges the walk's own state and
// the later block's first index) writes first_frame / last_frame of its label.  Every element has one writer: no atomics.
// The result of hypothesis (b, n) is a function of its own labels and of the ring and statistics rows of utterance b, which
// are the same bits for every group, position and N: no hypothesis can see another.
#include <type_traits>

#include "ctc_common.h"
#include "ctc_lane_ops.h"
#include "ctc_launch.h"
#include "ctc_nbest_align.h"

namespace ctc {
namespace {

constexpr int NBA_PW = 4;                               // producer wavefronts
constexpr int NBA_PT = 64 * NBA_PW;                     // producer threads
constexpr int NBA_THREADS = 64 * NBEST_G + NBA_PT;      // 768
constexpr int NBA_RING = 1024;                          // label emissions per hypothesis and ring buffer: frames per block = 1024 / UP
constexpr int NBA_WALK_BYTES = 4096;                    // one walk buffer (two per hypothesis): BF frames x 64 lanes x word

// back-pointer word of one lane and frame: 3 bits per label position (classic; simplified uses 1), NL positions
template <int NL> struct NbaWord { typedef unsigned char type; };
template <> struct NbaWord<4> { typedef unsigned short type; };
template <> struct NbaWord<8> { typedef unsigned int type; };
template <> struct NbaWord<16> { typedef unsigned long long type; };
constexpr int nba_word_bytes(int NL) { return NL <= 2 ? 1 : NL / 2; }

__device__ __forceinline__ float4 nba_row_load4(const char *row, int k, int dt) {
  if (dt == 0) return *reinterpret_cast<const float4 *>(row + (size_t)k * 4);
  const uint2 u = *reinterpret_cast<const uint2 *>(row + (size_t)k * 2);
  return make_float4(h16_to_f32((unsigned short)(u.x & 0xffffu), dt), h16_to_f32((unsigned short)(u.x >> 16), dt),
                     h16_to_f32((unsigned short)(u.y & 0xffffu), dt), h16_to_f32((unsigned short)(u.y >> 16), dt));
}
// the same four elements one by one (unaligned rows, V no multiple of 4): -inf past the row, which adds nothing to either statistic
__device__ __forceinline__ float4 nba_row_load4_elem(const char *row, int k, int V, int dt) {
  const float ninf = -__builtin_inff();
  return make_float4(row_load1(row, k, dt), k + 1 < V ? row_load1(row, k + 1, dt) : ninf, k + 2 < V ? row_load1(row, k + 2, dt) : ninf,
                     k + 3 < V ? row_load1(row, k + 3, dt) : ninf);
}
// running (max, sum of exp(x - max)) of one lane: four more elements (both access paths end here: identical bits)
__device__ __forceinline__ void nba_stat_add4(float &m, float &s, const float4 v) {
  const float mn = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
  s = s * fexp2((m - mn) * LOG2E) +
      ((fexp2((v.x - mn) * LOG2E) + fexp2((v.y - mn) * LOG2E)) + (fexp2((v.z - mn) * LOG2E) + fexp2((v.w - mn) * LOG2E)));
  m = mn;
}

// the token of label position i of hypothesis row `row` with L labels, -1 where nothing can be emitted
__device__ __forceinline__ int nba_token(const Problem &p, long row, int L, int i) {
  if (i < 0 || i >= L) return -1;
  const int tok = label_at(p, p.labels + row * p.label_stride, i);
  return emits(p, tok) ? tok : -1;
}

__device__ __forceinline__ double nba_readlane(double v, int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

template <int KIND, int NL>
__global__ __launch_bounds__(NBA_THREADS) void nbest_align_kernel(const Problem p, const int N, char *__restrict__ ws,
                                                                  float *__restrict__ score, int *__restrict__ tokens,
                                                                  int *__restrict__ label_index, int *__restrict__ first_frame,
                                                                  int *__restrict__ last_frame) {
  typedef typename NbaWord<NL>::type Word;
  typedef typename std::conditional<NL == 16, unsigned long long, unsigned int>::type Bits;
  constexpr int UP = 64 * NL;
  constexpr int F = NBA_RING / UP;                    // frames per ring buffer: 16, 8, 4, 2, 1
  constexpr int FR = NBEST_G * UP;                    // ring floats per frame: the eight hypotheses' emissions
  constexpr int CNT = FR / NBA_PT;                    // gathers per producer thread and frame: 2 NL
  constexpr int FPW = F / NBA_PW > 0 ? F / NBA_PW : 1;  // frames per producer wavefront and block, all in flight together
  constexpr int BF = NBA_WALK_BYTES / (64 * (int)sizeof(Word));  // frames per back-trace block: 64, 64, 32, 16, 8
  static_assert(2 * F * FR * 4 == 2 * NBEST_G * NBA_WALK_BYTES, "the walk buffers take the ring's place");
  static_assert(BF * 64 * (int)sizeof(Word) / 16 == NBA_PT, "one 16-byte piece of a walk block per producer thread and hypothesis");
  const double NINF = -__builtin_inf();

  __shared__ __attribute__((aligned(16))) float ring[2 * F * FR];  // [buffer][frame][hypothesis][position]; then the walk buffers
  __shared__ __attribute__((aligned(16))) float stat[2 * F * 4];   // [buffer][frame]: x[blank], row max, log2 sum exp(x - max)

  const int b = blockIdx.x, n0 = blockIdx.y * NBEST_G;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool chain = wave < NBEST_G;
  const int T = p.T, V = p.V, blank = p.blank, dt = p.xdtype;
  const int Tb = frame_count(p, b);
  const int esz = dt == 0 ? 4 : 2;
  const char *const xb = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb) * esz;
  // vector row accesses (16 bytes of float32, 8 bytes of 16-bit elements) need aligned rows; element-wise otherwise
  const bool vec = ((V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (dt == 0 ? 15 : 7)) == 0;

  // label count of hypothesis n of this utterance: 0 when there is none or it has too many labels (reported -inf at the end)
  auto count_of = [&](int n, bool &too_long) {
    too_long = false;
    if (n >= N) return 0;
    const int L = label_count(p, b * N + n);
    too_long = too_many_labels(p, L);
    return too_long ? 0 : L;
  };
  // the back-pointer rows of hypothesis row h: [T][64] words
  auto bp_of = [&](long h) { return reinterpret_cast<Word *>(ws) + (size_t)h * T * 64; };

  const int nb = (Tb + F - 1) / F;
  // what the back-trace of this chain starts from (chains only)
  const int n = n0 + wave;
  const long hrow = (long)b * N + n;
  bool feasible = false;
  int si = -1, sopen = 0;

  // The two roles run their own loops (the branch is wavefront-uniform) and meet at one raw barrier per block of frames.
  if (chain) {
    // ---- the chains (waves 0..7) ----
    bool too_long = false;
    const int L = __builtin_amdgcn_readfirstlane(count_of(n, too_long));
    double O[NL], C[NL];  // simplified: C is S, O unused
    unsigned allow = 0;   // classic: bit j = label[i] differs from label[i-1]
    double cs = 0.0;      // the start state: blank so far
    double lse = 0.0;     // sum of the frames' log-sum-exps, in frame order
#pragma unroll
    for (int j = 0; j < NL; ++j) { O[j] = NINF; C[j] = NINF; }
    if (KIND == 0) {
      int prev = nba_token(p, hrow, L, lane * NL - 1);
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const int i = lane * NL + j;
        const int tok = nba_token(p, hrow, L, i);
        if (i > 0 && tok != prev) allow |= 1u << j;
        prev = tok;
      }
    }
    Word *const bp = bp_of(n < N ? hrow : 0);  // (n >= N: never dereferenced)

    auto consume = [&](int kb) {
      const int t0 = kb * F;
      const int nf = Tb - t0 < F ? Tb - t0 : F;
      const float *const rb = ring + (kb & 1) * F * FR + wave * UP + lane * NL;
      const float *const sb = stat + (kb & 1) * F * 4;
      for (int f = 0; f < nf; ++f) {
        float e[NL];
        fused::ld_slots<NL>(rb + f * FR, e);
        const float4 sv = *reinterpret_cast<const float4 *>(sb + f * 4);
        const double ebd = (double)sv.x;
        lse += (double)sv.y + (double)sv.z * LN2_D;
        Bits bits = 0;
        if (KIND == 0) {
          const double pO = from_prev_lane(O[NL - 1], NINF);
          const double pC = from_prev_lane(C[NL - 1], cs);
#pragma unroll
          for (int j = NL - 1; j >= 0; --j) {
            const double qO = j > 0 ? O[j > 0 ? j - 1 : 0] : pO;
            const double qC = j > 0 ? C[j > 0 ? j - 1 : 0] : pC;
            const double a2 = ((allow >> j) & 1u) ? qO : NINF;
            double best = O[j];
            unsigned src = 0;
            if (qC > best) { best = qC; src = 1; }
            if (a2 > best) { best = a2; src = 2; }
            const unsigned sc = O[j] > C[j] ? 1u : 0u;
            const double bc = sc ? O[j] : C[j];
            O[j] = best + (double)e[j];
            C[j] = bc + ebd;
            bits |= (Bits)(src | (sc << 2)) << (3 * j);
          }
        } else {
          const double pS = from_prev_lane(C[NL - 1], cs);
#pragma unroll
          for (int j = NL - 1; j >= 0; --j) {
            const double q = j > 0 ? C[j > 0 ? j - 1 : 0] : pS;
            const double d = q + (double)e[j], h = C[j] + ebd;
            const unsigned sd = d > h ? 1u : 0u;
            C[j] = sd ? d : h;
            bits |= (Bits)sd << j;
          }
        }
        cs += ebd;
        bp[(size_t)(t0 + f) * 64 + lane] = (Word)bits;
      }
    };

    fused::block_barrier();
    for (int kb = 0; kb < nb; ++kb) {
      if (n < N) consume(kb);
      fused::block_barrier();
    }

    // the end state, the score and everything that is -1
    if (n < N) {
      const int i = L - 1, jj = i & (NL - 1);
      double cv = C[0], ov = O[0];
#pragma unroll
      for (int j = 1; j < NL; ++j)
        if (j == jj) { cv = C[j]; ov = O[j]; }
      double best = cs;
      if (L > 0) {
        const int op = KIND == 0 && ov > cv ? 1 : 0;
        const int src = __builtin_amdgcn_readfirstlane(i / NL);
        best = nba_readlane(op ? ov : cv, src);
        sopen = __builtin_amdgcn_readlane(op, src);
      }
      feasible = !too_long && best > NINF;
      si = L - 1;
      if (lane == 0) score[hrow] = (float)(feasible ? (p.wrt == 0 ? best - lse : best) : NINF);
      int *const tok_out = tokens + (size_t)hrow * T;
      int *const idx_out = label_index ? label_index + (size_t)hrow * T : nullptr;
      for (int t = (feasible ? Tb : 0) + lane; t < T; t += 64) {
        tok_out[t] = -1;
        if (idx_out) idx_out[t] = -1;
      }
      for (int k = (feasible ? L : 0) + lane; k < p.U; k += 64) {
        if (first_frame) first_frame[(size_t)hrow * p.U + k] = -1;
        if (last_frame) last_frame[(size_t)hrow * p.U + k] = -1;
      }
    }
  } else {
    // ---- the producers (waves 8..11): the labels a thread gathers are the same every frame ----
    const int tp = tid - 64 * NBEST_G, pw = wave - NBEST_G;
    unsigned goff[CNT];   // byte offset of the label's element in a row (the blank's where nothing can be emitted: a valid address)
    unsigned gvalid = 0;  // bit c: gather c is an emission
#pragma unroll
    for (int c = 0; c < CNT; ++c) {
      const int idx = tp + NBA_PT * c, g = idx / UP, i = idx % UP;
      bool tl;
      const int Lg = count_of(n0 + g, tl);
      const int tok = nba_token(p, (long)b * N + n0 + g, Lg, i);
      goff[c] = (unsigned)(tok >= 0 ? tok : blank) * (unsigned)esz;
      if (tok >= 0) gvalid |= 1u << c;
    }
    // the row of a block's position; past the utterance's end its last, valid memory whose results are never stored
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
          if (t0 + f < Tb) rb[f * FR + tp + NBA_PT * c] = e[k];
        }
      }
      // row statistics: this wavefront's frames f = pw + 4 q
      const char *row[FPW];
      float m[FPW], s[FPW], ebl[FPW];
#pragma unroll
      for (int q = 0; q < FPW; ++q) {
        const int f = pw + NBA_PW * q;
        row[q] = frame_row(f < F ? t0 + f : Tb);
        ebl[q] = row_load1(row[q], blank, dt);
        m[q] = -3.402823466e38f; s[q] = 0.f;
      }
      if (p.wrt == 0) {
        for (int k = lane * 4; k < V; k += 256) {
          float4 v[FPW];
#pragma unroll
          for (int q = 0; q < FPW; ++q) v[q] = vec ? nba_row_load4(row[q], k, dt) : nba_row_load4_elem(row[q], k, V, dt);
#pragma unroll
          for (int q = 0; q < FPW; ++q) nba_stat_add4(m[q], s[q], v[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < FPW; ++q) {
        const int f = pw + NBA_PW * q;
        float M = 0.f, l2s = 0.f;
        if (p.wrt == 0) {
          M = wave_max(m[q]);
          const float S = wave_sum(s[q] * fexp2((m[q] - M) * LOG2E));
          l2s = flog2(S);
          if (!(S > 0.f)) { M = 0.f; l2s = __builtin_inff(); }  // a row of -inf: no path through the frame has a finite value
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

  // every chain's back-pointer stores are done and visible to the producers, and the ring is free
  __syncthreads();
  if (Tb == 0) return;

  // ---- the back-trace ----
  char *const tb = reinterpret_cast<char *>(ring);  // [hypothesis][buffer][BF][64] words
  const int nblk = (Tb + BF - 1) / BF;
  if (chain) {
    const Word *const wbuf = reinterpret_cast<const Word *>(tb + wave * 2 * NBA_WALK_BYTES);
    const int32_t *const lab = p.labels + hrow * p.label_stride;  // (dereferenced by a feasible hypothesis only)
    int *const tok_out = tokens + (size_t)hrow * T;
    int *const idx_out = label_index ? label_index + (size_t)hrow * T : nullptr;
    int *const ff = first_frame ? first_frame + (size_t)hrow * p.U : nullptr;
    int *const lf = last_frame ? last_frame + (size_t)hrow * p.U : nullptr;
    int carry = -1;  // label index of the first frame of the block behind this one
    fused::block_barrier();
    for (int blk = nblk - 1; blk >= 0; --blk) {
      if (feasible) {
        const int f0 = blk * BF;
        const int nf = Tb - f0 < BF ? Tb - f0 : BF;
        const Word *const w = wbuf + (blk & 1) * BF * 64;
        int myidx = -1;
        for (int fl = nf - 1; fl >= 0; --fl) {
          int idx = -1;
          if (si >= 0) {
            const Word word = w[fl * 64 + si / NL];
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
        // the neighbours' label indices: frame f0 - 1 is what the walk's state says (open: it emitted label si)
        const int prv = fused::from_prev_lane_i(myidx, sopen ? si : -1);
        int nxt = fused::from_next_lane_i(myidx, -1);
        if (lane == nf - 1) nxt = carry;
        carry = __builtin_amdgcn_readlane(myidx, 0);
        if (lane < nf) {
          const int f = f0 + lane;
          tok_out[f] = myidx >= 0 ? label_at(p, lab, myidx) : blank;
          if (idx_out) idx_out[f] = myidx;
          if (myidx >= 0) {
            if (ff && (KIND == 1 || prv != myidx)) ff[myidx] = f;
            if (lf && (KIND == 1 || nxt != myidx)) lf[myidx] = f;
          }
        }
      }
      fused::block_barrier();
    }
  } else {
    const int tp = tid - 64 * NBEST_G;
    typedef unsigned int Piece __attribute__((ext_vector_type(4)));  // 16 bytes (a plain vector: the eight stay in registers)
    auto fetch = [&](int blk) {
      const int f0 = blk * BF;
      const int nf = Tb - f0 < BF ? Tb - f0 : BF;
      const int n16 = nf * 64 * (int)sizeof(Word) / 16;  // (rows are 64 * sizeof(Word) bytes: multiples of 64)
      // (every hypothesis' piece is loaded, from an address that is always valid, and stored: the eight loads are in flight
      // together in registers, and a buffer whose hypothesis does not exist or is infeasible is never walked)
      const int k = tp < n16 ? tp : n16 - 1;
      Piece v[NBEST_G];
#pragma unroll
      for (int g = 0; g < NBEST_G; ++g)
        v[g] = reinterpret_cast<const Piece *>(bp_of((long)b * N + (n0 + g < N ? n0 + g : n0)) + (size_t)f0 * 64)[k];
      if (tp < n16) {
#pragma unroll
        for (int g = 0; g < NBEST_G; ++g) reinterpret_cast<Piece *>(tb + (g * 2 + (blk & 1)) * NBA_WALK_BYTES)[tp] = v[g];
      }
    };
    fetch(nblk - 1);
    fused::block_barrier();
    for (int blk = nblk - 1; blk >= 0; --blk) {
      if (blk > 0) fetch(blk - 1);
      fused::block_barrier();
    }
  }
}

template <int KIND, int NL>
hipError_t launch_nbest_align(const Problem &p, int N, char *ws, float *score, int *tokens, int *label_index, int *first_frame,
                              int *last_frame, hipStream_t st) {
  hipLaunchKernelGGL((nbest_align_kernel<KIND, NL>), dim3(p.B, (N + NBEST_G - 1) / NBEST_G), dim3(NBA_THREADS), 0, st, p, N, ws, score,
                     tokens, label_index, first_frame, last_frame);
  return hipGetLastError();
}

}  // namespace

size_t nbest_align_workspace_bytes(int B, int T, int U, int N) {
  return ((size_t)B * N * T * 64 * nba_word_bytes(nl_for(U)) + 255) & ~size_t(255);
}

hipError_t run_nbest_align(const Problem &p, int N, char *ws, float *score, int *tokens, int *label_index, int *first_frame,
                           int *last_frame, hipStream_t st) {
  typedef hipError_t Launch(const Problem &, int, char *, float *, int *, int *, int *, int *, hipStream_t);
  static Launch *const table[2][5] = {
      {launch_nbest_align<0, 1>, launch_nbest_align<0, 2>, launch_nbest_align<0, 4>, launch_nbest_align<0, 8>, launch_nbest_align<0, 16>},
      {launch_nbest_align<1, 1>, launch_nbest_align<1, 2>, launch_nbest_align<1, 4>, launch_nbest_align<1, 8>, launch_nbest_align<1, 16>}};
  const int NL = nl_for(p.U);
  const int lg = NL == 1 ? 0 : NL == 2 ? 1 : NL == 4 ? 2 : NL == 8 ? 3 : NL == 16 ? 4 : -1;
  if (lg < 0 || p.kind < 0 || p.kind > 1 || N < 1) return hipErrorInvalidValue;
  return table[p.kind][lg](p, N, ws, score, tokens, label_index, first_frame, last_frame, st);
}

}  // namespace ctc
