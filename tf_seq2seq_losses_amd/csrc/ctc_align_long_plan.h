// Host-side plan of the tiled best-path alignment (ctc_align_long.hip, ctc_amd_long_best_path): the tile grid, the launch schedule
// and the workspace offsets.  Plain C++ with no HIP in it, so that tests/tools/long_plan_check.cpp can run it under the host
// sanitizers.  Every byte count is a size_t: B * K * T * 512 passes 2^31 at realistic sizes.
#pragma once
#include <stddef.h>

namespace ctc {

constexpr int LONG_NL = 16;                   // label positions per lane: the chain step of align_kernel<KIND, 16>
constexpr int LONG_UB = 64 * LONG_NL;         // label positions per label block
constexpr int LONG_RING_FRAMES = 4096 / LONG_UB;  // frames per ring block (= ALIGN_RING / UB): frames_per_tile is a multiple of it
constexpr int LONG_TF_DEFAULT = 128;          // frames per tile when the caller passes 0
constexpr int LONG_MAX_U = 65536;             // = CTC_AMD_LONG_MAX_U
constexpr int LONG_ROW_DOUBLES = 2 * LONG_UB + 8;  // row buffer of one (utterance, label block): O, C per position, then the start state

struct LongPlan {
  int B, T, U;
  int K, J, TF;       // label blocks, time blocks, frames per tile
  int launches;       // K + J - 1 anti-diagonals of tiles (then the trace and, on request, the per-label frames)
  size_t off_bp, off_col, off_row, off_lse, off_idx, off_flag, total;
};

inline size_t long_r256(size_t x) { return (x + 255) & ~size_t(255); }

// false: frames_per_tile is neither 0 nor a positive multiple of LONG_RING_FRAMES, a size is negative or beyond the limit, or a
// launch grid would pass 2^31 - 1 workgroups
inline bool long_plan(int B, int T, int U, int frames_per_tile, LongPlan *out) {
  if (B < 0 || T < 0 || U < 0 || U > LONG_MAX_U || frames_per_tile < 0 || frames_per_tile % LONG_RING_FRAMES != 0) return false;
  LongPlan P;
  P.B = B; P.T = T; P.U = U;
  P.TF = frames_per_tile ? frames_per_tile : LONG_TF_DEFAULT;
  P.K = U > 0 ? (U + LONG_UB - 1) / LONG_UB : 1;
  P.J = T > 0 ? (int)(((long long)T + P.TF - 1) / P.TF) : 1;
  P.launches = P.K + P.J - 1;
  const size_t b = (size_t)B, t = (size_t)T, k = (size_t)P.K;
  // the widest grids: a full diagonal of tiles per utterance, and 256 frames or labels per workgroup of the per-label kernel
  const size_t diag = (size_t)(P.K < P.J ? P.K : P.J), per_label = ((size_t)(T > U ? T : U) + 255) / 256;
  if (b * diag > 2147483647u || b * per_label > 2147483647u) return false;
  size_t o = 0;
  P.off_bp = o;   o = long_r256(o + b * k * t * 64 * 8);             // back-pointers: [B][K][T][64] words of 8 bytes
  P.off_col = o;  o = long_r256(o + b * (k - 1) * t * 16);           // columns: [B][K - 1][T] pairs (O, C) of float64
  P.off_row = o;  o = long_r256(o + b * k * LONG_ROW_DOUBLES * 8);   // rows: [B][K] chain states
  P.off_lse = o;  o = long_r256(o + b * (size_t)P.J * 8);            // LSE partials: [B][J] float64
  P.off_idx = o;  o = long_r256(o + b * t * 4);                      // label_index when the caller passes none: [B][T] int32
  P.off_flag = o; o = long_r256(o + b * 4);                          // feasible: [B] int32
  P.total = o;
  *out = P;
  return true;
}

// launch d of 0 .. launches - 1 runs the tiles (k, d - k), k = *k_lo .. *k_lo + *count - 1, of every utterance
inline void long_diagonal(const LongPlan &P, int d, int *k_lo, int *count) {
  const int lo = d - (P.J - 1) > 0 ? d - (P.J - 1) : 0, hi = d < P.K - 1 ? d : P.K - 1;
  *k_lo = lo;
  *count = hi - lo + 1;
}

}  // namespace ctc
