// Host-side plan of the tiled edit counts (ctc_edit_long.hip, ctc_amd_edit_counts): the tile grid, the launch schedule and the
// workspace offsets.  Plain C++ with no HIP in it, so that tests/tools/edit_counts_plan_check.cpp can run it under the host
// sanitizers.  Every byte count is a size_t: B * N * (K - 1) * hyp_stride * 8 passes 2^32 at realistic sizes.
#pragma once
#include <stddef.h>

namespace ctc {

constexpr int EDIT_LONG_NL = 16;                  // reference tokens per lane of a full column block
constexpr int EDIT_LONG_UB = 64 * EDIT_LONG_NL;   // reference tokens per column block
constexpr int EDIT_LONG_ROWS_MULTIPLE = 64;       // rows_per_tile is a multiple of the hypothesis token chunk
constexpr int EDIT_LONG_RT_DEFAULT = 256;         // hypothesis tokens per tile when the caller passes 0 (profiles/edit_counts_time.md)
constexpr int EDIT_LONG_MAX_R = 65536;            // = CTC_AMD_LONG_MAX_U
constexpr int EDIT_LONG_MAX_STRIDE = 1 << 20;     // = CTC_AMD_EDIT_COUNTS_MAX_STRIDE: d, S and I each fit 21 bits of the packed word
constexpr int EDIT_LONG_WAVES = 4;                // tiles per workgroup

struct EditCountsPlan {
  int B, N, R, hyp_stride;
  int NL;             // reference tokens per lane: the smallest power of two with 64 * NL >= R, at most 16 (K == 1 below 16)
  int K, J, RT;       // column blocks, row blocks, hypothesis tokens per tile
  int launches;       // K + J - 1 anti-diagonals of tiles
  size_t off_col, off_row, total;
};

inline size_t edit_long_r256(size_t x) { return (x + 255) & ~size_t(255); }

// false: rows_per_tile is neither 0 nor a positive multiple of 64, a size is negative or beyond its limit, N < 1, B * N >= 2^31 or
// a launch grid would pass 2^31 - 1 workgroups
inline bool edit_counts_plan(int B, int N, int R, int hyp_stride, int rows_per_tile, EditCountsPlan *out) {
  if (B < 0 || N < 1 || R < 0 || R > EDIT_LONG_MAX_R || hyp_stride < 0 || hyp_stride > EDIT_LONG_MAX_STRIDE) return false;
  if (rows_per_tile < 0 || rows_per_tile % EDIT_LONG_ROWS_MULTIPLE != 0) return false;
  const size_t pairs = (size_t)B * (size_t)N;
  if (pairs > 2147483647u) return false;
  EditCountsPlan P;
  P.B = B; P.N = N; P.R = R; P.hyp_stride = hyp_stride;
  P.NL = 1;
  while (P.NL < EDIT_LONG_NL && 64 * P.NL < R) P.NL *= 2;
  P.RT = rows_per_tile ? rows_per_tile : EDIT_LONG_RT_DEFAULT;
  P.K = R > 0 ? (R + EDIT_LONG_UB - 1) / EDIT_LONG_UB : 1;
  P.J = hyp_stride > 0 ? (int)(((long long)hyp_stride + P.RT - 1) / P.RT) : 1;
  P.launches = P.K + P.J - 1;
  // the widest grid: a full diagonal of tiles per pair, EDIT_LONG_WAVES tiles per workgroup
  const size_t diag = (size_t)(P.K < P.J ? P.K : P.J);
  if ((pairs * diag + EDIT_LONG_WAVES - 1) / EDIT_LONG_WAVES > 2147483647u) return false;
  const size_t k = (size_t)P.K;
  size_t o = 0;
  P.off_col = o; o = edit_long_r256(o + pairs * (k - 1) * (size_t)hyp_stride * 8);  // columns: [B * N][K - 1][hyp_stride] packed words
  P.off_row = o; o = edit_long_r256(o + pairs * k * EDIT_LONG_UB * 8);              // rows: [B * N][K][1024] packed words
  P.total = o;
  *out = P;
  return true;
}

// launch d of 0 .. launches - 1 runs the tiles (k, d - k), k = *k_lo .. *k_lo + *count - 1, of every pair
inline void edit_counts_diagonal(const EditCountsPlan &P, int d, int *k_lo, int *count) {
  const int lo = d - (P.J - 1) > 0 ? d - (P.J - 1) : 0, hi = d < P.K - 1 ? d : P.K - 1;
  *k_lo = lo;
  *count = hi - lo + 1;
}

}  // namespace ctc
