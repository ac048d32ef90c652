// Host-side plan of the tiled best-path alignment with optional wildcards and the exclusion of the next label
// (ctc_align_long_star.hip, ctc_amd_long_optional_wildcard_best_path / ctc_amd_long_star_best_path): the
// regions of ctc_align_long_wild_plan.h for the unit's own label block -- UB = 512 positions on the classic lattice (8 per lane),
// 1024 on the simplified one (16 per lane), back-pointer words of 4 bytes on both -- and behind them three more buffers.  Plain C++
// with no HIP in it; every byte count is a size_t.
//
// With K = max(1, ceil(U / UB)) label blocks, J = max(1, ceil(T / TF)) time blocks and r(x) = x rounded up to 256 bytes:
//   total = r(B K T 64 4) + r(B (K - 1) T 16) + r(B K (2 UB + 8) 8) + r(B J 8) + r(B T 4) + r(B 4)      the regions of long_plan
//         + r(B T 8) + r(B T 4) + r(B T 8)                                                             ... and of long_wild_plan
//         + r(B (K - 1) T 16)      the second column: the states of position k UB - 2 before every frame
//         + r(B T 8)               m2, the best emission of a token other than k1, of every frame
//         + r(B T 4)               k2, the lowest token that attains it
// One plan serves every combination of the two keywords (a call without the exclusion leaves the last two buffers alone, one
// without optional wildcards the second column).
#pragma once
#include <stddef.h>

#include "ctc_align_long_wild_plan.h"

#if defined(__HIPCC__)
#define CTC_LS_HD __host__ __device__ inline
#else
#define CTC_LS_HD inline
#endif

namespace ctc {

constexpr int LONG_STAR_WORD_BYTES = 4;  // classic: 3 source bits and 1 open/closed bit for 8 positions; simplified: 1 + 1 bits for 16
constexpr int long_star_nl(int kind) { return kind == 0 ? 8 : 16; }
constexpr int long_star_block(int kind) { return 64 * long_star_nl(kind); }
constexpr int long_star_row_doubles(int UB) { return 2 * UB + 8; }  // O, C per position, then the start state

struct LongStarPlan {
  LongPlan base;  // K, J, TF, launches and the six regions of long_plan for blocks of UB positions; base.total: where the rest begins
  int UB;
  size_t off_max, off_arg, off_lp, off_col2, off_max2, off_arg2, total;
};

// Which tiles run: a function of (Tb, L, k, j, TF) and the unit's block size alone.  A tile that does not run writes nothing, and
// nothing of it is read: the trace asks the same function before it reads a row buffer.  Without optional wildcards every position
// takes a frame (the tests of ctc_align_long_wild.hip); with them no two such positions are adjacent, so position i is -inf before
// frame i / 2 and L positions need L / 2 frames (those of long_loss_tile_active_opt).  What is infeasible beyond the count falls out
// of the lattice as an end state of -inf.
CTC_LS_HD bool long_star_refused(bool opt, int Tb, int L) { return opt ? L / 2 > Tb : L > Tb; }
CTC_LS_HD bool long_star_tile_active(bool opt, int Tb, int L, int k, int j, int TF, int UB) {
  if (long_star_refused(opt, Tb, L)) return false;
  if ((long long)j * TF >= Tb) return false;
  if (k > 0 && (long long)k * UB >= L) return false;
  if ((long long)j * TF + TF - 1 < (long long)k * UB / (opt ? 2 : 1)) return false;
  return true;
}
// (for a tile that runs) the block's first tile starts from -inf: the tile before it in time did not run
CTC_LS_HD bool long_star_fresh(bool opt, int k, int j, int TF, int UB) { return (long long)j * TF <= (long long)k * UB / (opt ? 2 : 1); }

// false: what long_plan refuses, or a launch grid of more than 2^31 - 1 workgroups with this unit's narrower blocks
inline bool long_star_plan(int kind, int B, int T, int U, int frames_per_tile, LongStarPlan *out) {
  LongStarPlan S;
  if (kind < 0 || kind > 1 || !long_plan(B, T, U, frames_per_tile, &S.base)) return false;
  LongPlan &P = S.base;
  const int UB = long_star_block(kind);
  S.UB = UB;
  P.K = U > 0 ? (U + UB - 1) / UB : 1;
  P.launches = P.K + P.J - 1;
  const size_t b = (size_t)B, t = (size_t)T, k = (size_t)P.K;
  if (b * (size_t)(P.K < P.J ? P.K : P.J) > 2147483647u) return false;
  size_t o = 0;
  P.off_bp = o;   o = long_r256(o + b * k * t * 64 * LONG_STAR_WORD_BYTES);       // back-pointers: [B][K][T][64] words
  P.off_col = o;  o = long_r256(o + b * (k - 1) * t * 16);                        // columns: [B][K - 1][T] pairs (O, C) of position k UB - 1
  P.off_row = o;  o = long_r256(o + b * k * (size_t)long_star_row_doubles(UB) * 8);  // rows: [B][K] chain states
  P.off_lse = o;  o = long_r256(o + b * (size_t)P.J * 8);                         // LSE partials: [B][J] float64
  P.off_idx = o;  o = long_r256(o + b * t * 4);                                   // label_index when the caller passes none
  P.off_flag = o; o = long_r256(o + b * 4);                                       // feasible: [B] int32
  P.total = o;
  S.off_max = o;  o = long_r256(o + b * t * 8);             // m1, the row maximum: [B][T] float64
  S.off_arg = o;  o = long_r256(o + b * t * 4);             // k1, the lowest token that attains it: [B][T] int32
  S.off_lp = o;   o = long_r256(o + b * t * 8);             // the sweep: LSE_t; the back-trace: lp[t, pi_t]: [B][T] float64
  S.off_col2 = o; o = long_r256(o + b * (k - 1) * t * 16);  // columns of position k UB - 2
  S.off_max2 = o; o = long_r256(o + b * t * 8);             // m2: [B][T] float64
  S.off_arg2 = o; o = long_r256(o + b * t * 4);             // k2: [B][T] int32
  S.total = o;
  *out = S;
  return true;
}

}  // namespace ctc
