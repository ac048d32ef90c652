// Edit counts -- distance, substitutions, insertions, deletions -- of N hypotheses per utterance against the utterance's reference,
// for references of up to 65536 tokens: ctc_amd_edit_counts (include/ctc_amd.h), DESIGN.md section 5.23.
//
// Every cell of the table of ctc_edit.hip carries the triple (d, S, I) packed into one signed 64-bit word d * 2^42 + S * 2^21 + I, so
// that the lexicographic minimum of three candidates is a signed minimum and a move is one addition:
//   up (insertion) + INS = 2^42 + 1, left (deletion) + DEL = 2^42, diagonal + 0 (equal tokens) or + SUB = 2^42 + 2^21.
// The decomposition inside a tile is that of ctc_edit.hip: one wavefront per pair, the reference along the lanes (NL positions per
// lane), the hypothesis the serial axis, the left neighbour and the hypothesis token by DPP shifts, tokens in chunks of 64 loaded
// one chunk ahead, no LDS, no barrier.  The table is tiled over column blocks of 64 * NL reference tokens x row blocks of RT
// hypothesis tokens; launch dg runs the tiles (k, dg - k) of every pair, so a tile's upper and left neighbours ran one launch
// earlier and no workgroup waits for another.
//   * Tile (k, jt) owns rows i0 + 1 .. i0 + RT (i0 = jt * RT) of columns j00 + 1 .. j00 + 64 * NL (j00 = k * 64 * NL).  It runs when
//     j00 < r and i0 < h; a pair with h == 0, r == 0 or r > R is answered by its tile (0, 0) alone.
//   * Top row: D[0][j] = j * DEL for jt == 0, else the bottom row of tile (k, jt - 1) from the workspace (rows[pair][k], each lane
//     its own NL words: the tile overwrites them in place when the tile below will run).
//   * Left column: lane 0 takes D[i][j00] out of a chunk of 64 words the way it takes the token: for k == 0 the chunk is computed
//     (i * INS), otherwise it is loaded from cols[pair][k - 1][i - 1], where lane 63 of tile (k - 1, jt) stored its last column of
//     every row.  The diagonal source of lane 0 in the tile's first row is the corner D[i0][j00]: j00 * DEL, i0 * INS or the entry
//     i0 - 1 of the same column, which tile (k - 1, jt - 1) stored two launches earlier.
//   * A tile runs rows + 63 steps (rows = min(RT, h - i0)), until every lane has done its last row; in the pair's last column block
//     it stops after the lane that holds column r, as nothing to the right of column r is ever read by a column <= r.
//   * The answer is slot (r - 1 - j00) % NL of lane (r - 1 - j00) / NL in the tile that holds cell (h, r): the only writer of counts.
#include "ctc_common.h"
#include "ctc_edit_long_plan.h"
#include "ctc_lane_ops.h"
#include "ctc_launch.h"

namespace ctc {
namespace {

using fused::from_prev_lane_i;
using fused::imax;
using fused::imin;
using fused::readlane_i;

typedef long long word;  // d * 2^42 + S * 2^21 + I
constexpr word EDIT_DEL = 1LL << 42, EDIT_SUB = EDIT_DEL + (1LL << 21), EDIT_INS = EDIT_DEL + 1;

__device__ __forceinline__ word wmin(word a, word b) { return a < b ? a : b; }
__device__ __forceinline__ word make_word(int lo, int hi) { return (word)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo); }
__device__ __forceinline__ word from_prev_lane_w(word x, word fill) {
  return make_word(from_prev_lane_i((int)x, (int)fill), from_prev_lane_i((int)(x >> 32), (int)(fill >> 32)));
}
__device__ __forceinline__ word readlane_w(word v, int l) { return make_word(readlane_i((int)v, l), readlane_i((int)(v >> 32), l)); }

// Steps s0 .. s0 + n - 1 (n <= 64, may be <= 0) of one tile: `chunk` holds the hypothesis tokens and `colchunk` the left boundary
// D[i][j00] of the rows i0 + s0 + 1 .. i0 + s0 + 64 along the lanes.  colq: where lane 63 stores its last column (row i0 + 1 at colq[0]).
template <int NL>
__device__ __forceinline__ void count_steps(int s0, int n, int chunk, word colchunk, int lane, int rows, const int (&rt)[NL], word (&d)[NL],
                                            word &left_up, int &tok, bool store_col, word *__restrict__ colq) {
  for (int k = 0; k < n; ++k) {
    const int s = s0 + k;
    tok = from_prev_lane_i(tok, readlane_i(chunk, k));
    const word left0 = from_prev_lane_w(d[NL - 1], readlane_w(colchunk, k));  // D[i][j0]
    if ((unsigned)(s - lane) < (unsigned)rows) {
      // off the chain: the two candidates that do not involve this row's left neighbour
      word c[NL], diag = left_up;
#pragma unroll
      for (int q = 0; q < NL; ++q) {
        c[q] = wmin(d[q] + EDIT_INS, diag + (tok != rt[q] ? EDIT_SUB : 0));
        diag = d[q];
      }
      word left = left0;
#pragma unroll
      for (int q = 0; q < NL; ++q) {
        left = wmin(left + EDIT_DEL, c[q]);
        d[q] = left;
      }
      left_up = left0;
      if (store_col && lane == 63) colq[s - 63] = left;
    }
  }
}

template <int NL>
__global__ __launch_bounds__(64 * EDIT_LONG_WAVES) void edit_counts_kernel(const int *__restrict__ hyp, int hyp_stride, const int *__restrict__ hyp_length,
                                                                           const int *__restrict__ ref, int ref_stride, const int *__restrict__ ref_length,
                                                                           int N, int R, int K, int RT, int dg, int k_lo, int count, long tiles,
                                                                           word *__restrict__ cols, word *__restrict__ rows, int *__restrict__ counts) {
  constexpr int UB = 64 * NL;
  const int lane = threadIdx.x & 63;
  const long wide = (long)blockIdx.x * EDIT_LONG_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (wide >= tiles) return;
  const int idx = (int)(wide / count);  // the pair (b, n); wave-uniform, as everything derived from it
  const int k = k_lo + (int)(wide % count), jt = dg - k;
  const int b = idx / N;
  const int h = __builtin_amdgcn_readfirstlane(imin(imax(hyp_length[idx], 0), hyp_stride));
  const int r = __builtin_amdgcn_readfirstlane(imin(imax(ref_length[b], 0), ref_stride));
  const bool origin = k == 0 && jt == 0;
  if (r > R) {  // beyond the bound the plan was made for
    if (origin && lane < 4) counts[4 * (size_t)idx + lane] = -1;
    return;
  }
  if (h == 0 || r == 0) {  // h insertions or r deletions
    if (origin && lane < 4) counts[4 * (size_t)idx + lane] = lane == 0 ? h + r : lane == 1 ? 0 : lane == 2 ? h : r;
    return;
  }
  const int j00 = k * UB, i0 = jt * RT;
  if (j00 >= r || i0 >= h) return;  // wholly beyond this pair's table

  const int *const hp = hyp + (size_t)idx * hyp_stride;
  const int *const rp = ref + (size_t)b * ref_stride;
  const word *const colp = cols + ((size_t)idx * (K - 1) + imax(k - 1, 0)) * hyp_stride;  // read when k > 0
  word *const rowp = rows + ((size_t)idx * K + k) * EDIT_LONG_UB + lane * NL;
  const int j0 = j00 + lane * NL;  // the column left of this lane's positions

  int rt[NL];
  word d[NL];  // reference tokens of the lane; row i - 1 of the lane (before its first row: the tile's top row)
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    rt[q] = j0 + q < r ? rp[j0 + q] : 0;  // columns beyond r are computed and never read: D[h][r] depends on columns <= r only
    d[q] = jt == 0 ? (word)(j0 + q + 1) * EDIT_DEL : rowp[q];
  }
  const word corner = jt == 0 ? (word)j00 * EDIT_DEL : k == 0 ? (word)i0 * EDIT_INS : colp[i0 - 1];  // D[i0][j00]
  word left_up = from_prev_lane_w(d[NL - 1], corner);                                                  // D[i - 1][j0]

  const int nrows = imin(RT, h - i0);
  const int kl = (r - 1) / UB;                               // the pair's last column block
  const int lanes = k == kl ? (r - 1 - j00) / NL : 63;       // the last lane anything reads
  const int steps = nrows + lanes;
  const bool store_col = k < kl;                             // the tile to the right runs
  word *const colq = cols + ((size_t)idx * (K - 1) + imin(k, imax(K - 2, 0))) * hyp_stride + i0;  // written when k < kl <= K - 1

  // Tokens and left-boundary words of the rows i0 + 64 c + 1 .. i0 + 64 c + 64 of an even chunk c and of the odd chunk behind it;
  // each is reloaded in place as soon as it is used up.  Every load is issued unconditionally (index clamped into the hypothesis:
  // rows beyond h are never used, and rows beyond this tile belong to a tile of the same launch and are never used either).
  auto token_chunk = [&](int s) { return hp[imin(i0 + s + lane, h - 1)]; };
  auto column_chunk = [&](int s) { return k == 0 ? (word)(i0 + s + lane + 1) * EDIT_INS : colp[imin(i0 + s + lane, h - 1)]; };
  int cur = token_chunk(0), nxt = token_chunk(64);
  word ccur = column_chunk(0), cnxt = column_chunk(64);
  int tok = 0;  // the hypothesis token of this lane's current row
  for (int s0 = 0; s0 < steps; s0 += 128) {
    count_steps<NL>(s0, imin(64, steps - s0), cur, ccur, lane, nrows, rt, d, left_up, tok, store_col, colq);
    cur = token_chunk(s0 + 128);
    ccur = column_chunk(s0 + 128);
    count_steps<NL>(s0 + 64, imin(64, steps - s0 - 64), nxt, cnxt, lane, nrows, rt, d, left_up, tok, store_col, colq);
    nxt = token_chunk(s0 + 192);
    cnxt = column_chunk(s0 + 192);
  }

  if (i0 + nrows < h) {  // the tile below runs: every lane has finished row i0 + RT, the row is un-skewed
#pragma unroll
    for (int q = 0; q < NL; ++q) rowp[q] = d[q];
  } else if (k == kl) {  // cell (h, r)
    const int slot = (r - 1 - j00) % NL;
    word sel = d[0];
#pragma unroll
    for (int q = 1; q < NL; ++q) sel = q == slot ? d[q] : sel;
    const word w = readlane_w(sel, lanes);
    const int dist = (int)(w >> 42), sub = (int)(w >> 21) & 0x1fffff, ins = (int)w & 0x1fffff;
    if (lane < 4) counts[4 * (size_t)idx + lane] = lane == 0 ? dist : lane == 1 ? sub : lane == 2 ? ins : dist - sub - ins;
  }
}

}  // namespace

hipError_t run_edit_counts(const int *hyp, int hyp_stride, const int *hyp_length, const int *ref, int ref_stride, const int *ref_length,
                           int N, const EditCountsPlan &P, int *counts, char *ws, hipStream_t st) {
  const long total = (long)P.B * N;
  if (total <= 0) return hipSuccess;
  word *const cols = reinterpret_cast<word *>(ws + P.off_col), *const rows = reinterpret_cast<word *>(ws + P.off_row);
  const dim3 block(64 * EDIT_LONG_WAVES);
  for (int dg = 0; dg < P.launches; ++dg) {
    int k_lo, count;
    edit_counts_diagonal(P, dg, &k_lo, &count);
    const long tiles = total * count;
    const dim3 grid((unsigned)((tiles + EDIT_LONG_WAVES - 1) / EDIT_LONG_WAVES));
#define CTC_EDIT_COUNTS_LAUNCH(NL)                                                                                                       \
  hipLaunchKernelGGL((edit_counts_kernel<NL>), grid, block, 0, st, hyp, hyp_stride, hyp_length, ref, ref_stride, ref_length, N, P.R, P.K, \
                     P.RT, dg, k_lo, count, tiles, cols, rows, counts)
    if (P.NL == 1) CTC_EDIT_COUNTS_LAUNCH(1);
    else if (P.NL == 2) CTC_EDIT_COUNTS_LAUNCH(2);
    else if (P.NL == 4) CTC_EDIT_COUNTS_LAUNCH(4);
    else if (P.NL == 8) CTC_EDIT_COUNTS_LAUNCH(8);
    else CTC_EDIT_COUNTS_LAUNCH(16);
#undef CTC_EDIT_COUNTS_LAUNCH
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

}  // namespace ctc
