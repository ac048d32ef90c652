// Edit (Levenshtein) distance of N hypotheses per utterance to the utterance's reference: ctc_amd_edit_distance (include/ctc_amd.h),
// DESIGN.md section 5.13.  Unit cost for insertion, deletion and substitution; tokens are arbitrary int32 values compared for equality.
//
// One launch, one wavefront per pair (b, n), EDIT_WAVES pairs per workgroup (nothing is shared between them: no LDS, no barrier).
//   * The reference lies along the lanes, NL consecutive positions per lane (NL = 1, 2, 4, 8, 16: the smallest power of two with
//     64 * NL >= R), loaded into registers once.  Lane l owns columns j = l * NL + 1 .. l * NL + NL of the table D[i][j].
//   * The hypothesis is the sequential axis.  At step s lane l computes row i = s - l + 1 of its columns, serially in-lane.  From lane
//     l - 1 it needs that lane's last column of row i, made at step s - 1 (one DPP shift per step), and the same column of row i - 1,
//     which it received one step earlier and keeps.  Lane 0's left neighbour is the boundary column D[i][0] = i; the top row is
//     D[0][j] = j.  A lane before its first row or after row h is predicated off: its state does not change.
//   * The hypothesis tokens travel down the lanes the same way (one more DPP shift per step).  Lane 0 takes token s out of a register
//     chunk of 64 tokens with a wave-uniform readlane; a chunk is loaded coalesced every 64 steps, one chunk ahead (two registers,
//     each reloaded in place when used up, by an unconditional load), so no step waits on a dependent global load.
//   * D[h][r] is slot (r - 1) % NL of lane (r - 1) / NL after that lane's row h: h + (r - 1) / NL steps, at most h + 63.
#include "ctc_common.h"
#include "ctc_lane_ops.h"
#include "ctc_launch.h"

namespace ctc {
namespace {

using fused::from_prev_lane_i;
using fused::imax;
using fused::imin;
using fused::readlane_i;

constexpr int EDIT_WAVES = 4;  // pairs per workgroup

// Steps s0 .. s0 + n - 1 (n <= 64, may be <= 0) of one wavefront: `chunk` holds the hypothesis tokens s0 .. s0 + 63 along the lanes.
template <int NL>
__device__ __forceinline__ void edit_steps(int s0, int n, int chunk, int lane, int h, const int (&rt)[NL], int (&d)[NL], int &left_up,
                                           int &tok) {
  for (int k = 0; k < n; ++k) {
    const int s = s0 + k;
    tok = from_prev_lane_i(tok, readlane_i(chunk, k));
    const int left0 = from_prev_lane_i(d[NL - 1], s + 1);  // D[i][j0]
    if ((unsigned)(s - lane) < (unsigned)h) {              // 1 <= i <= h
      // off the chain: the two candidates that do not involve this row's left neighbour
      int c[NL], diag = left_up;
#pragma unroll
      for (int q = 0; q < NL; ++q) {
        c[q] = imin(d[q] + 1, diag + (tok != rt[q] ? 1 : 0));
        diag = d[q];
      }
      int left = left0;
#pragma unroll
      for (int q = 0; q < NL; ++q) {
        left = imin(left + 1, c[q]);
        d[q] = left;
      }
      left_up = left0;
    }
  }
}

template <int NL>
__global__ __launch_bounds__(64 * EDIT_WAVES) void edit_kernel(const int *__restrict__ hyp, int hyp_stride, const int *__restrict__ hyp_length,
                                                               const int *__restrict__ ref, int ref_stride, const int *__restrict__ ref_length,
                                                               int N, int R, int total, int *__restrict__ distance) {
  const int lane = threadIdx.x & 63;
  const long wide = (long)blockIdx.x * EDIT_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (wide >= total) return;
  const int idx = (int)wide;  // the pair (b, n); wave-uniform, as everything derived from it
  const int b = idx / N;
  const int h = __builtin_amdgcn_readfirstlane(imin(imax(hyp_length[idx], 0), hyp_stride));
  const int r = __builtin_amdgcn_readfirstlane(imin(imax(ref_length[b], 0), ref_stride));
  if (r > R) {  // beyond the bound the instantiation was chosen for
    if (lane == 0) distance[idx] = -1;
    return;
  }
  const int *const hp = hyp + (size_t)idx * hyp_stride;
  const int *const rp = ref + (size_t)b * ref_stride;
  const int j0 = lane * NL;  // the column left of this lane's block

  int rt[NL], d[NL];  // reference tokens of the block; row i - 1 of the block (before a lane's first row: the top row)
#pragma unroll
  for (int q = 0; q < NL; ++q) {
    rt[q] = j0 + q < r ? rp[j0 + q] : 0;  // columns beyond r are computed and never read: D[h][r] depends on columns <= r only
    d[q] = j0 + q + 1;
  }
  int left_up = j0;  // D[i - 1][j0]

  const int last = r > 0 ? (r - 1) / NL : 0;  // the lane that holds D[.][r]
  const int steps = (h > 0 && r > 0) ? h + last : 0;
  if (steps > 0) {
    // Tokens 64 c .. 64 c + 63 of an even chunk c and of the odd chunk behind it; each is reloaded in place as soon as it is used up.
    // Every load is issued unconditionally (index clamped into the hypothesis: tokens at and beyond h are never used), so the loads
    // in flight are countable and a step waits for the chunk in use only, never for the load that has just been issued.
    int cur = hp[imin(lane, h - 1)], nxt = hp[imin(64 + lane, h - 1)];
    int tok = 0;  // the hypothesis token of this lane's current row
    for (int s0 = 0; s0 < steps; s0 += 128) {
      edit_steps<NL>(s0, imin(64, steps - s0), cur, lane, h, rt, d, left_up, tok);
      cur = hp[imin(s0 + 128 + lane, h - 1)];
      edit_steps<NL>(s0 + 64, imin(64, steps - s0 - 64), nxt, lane, h, rt, d, left_up, tok);
      nxt = hp[imin(s0 + 192 + lane, h - 1)];
    }
  }

  int out = h;  // r == 0
  if (r > 0) {
    const int slot = (r - 1) % NL;
    int sel = d[0];
#pragma unroll
    for (int q = 1; q < NL; ++q) sel = q == slot ? d[q] : sel;
    out = readlane_i(sel, last);
  }
  if (lane == 0) distance[idx] = out;
}

}  // namespace

hipError_t run_edit_distance(const int *hyp, int hyp_stride, const int *hyp_length, const int *ref, int ref_stride, const int *ref_length,
                             int B, int N, int R, int *distance, hipStream_t st) {
  const long total = (long)B * N;
  if (total <= 0 || total > 0x7fffffffL) return total == 0 ? hipSuccess : hipErrorInvalidValue;
  const dim3 grid((unsigned)((total + EDIT_WAVES - 1) / EDIT_WAVES)), block(64 * EDIT_WAVES);
#define CTC_EDIT_LAUNCH(NL) \
  hipLaunchKernelGGL((edit_kernel<NL>), grid, block, 0, st, hyp, hyp_stride, hyp_length, ref, ref_stride, ref_length, N, R, (int)total, distance)
  if (R <= 64) CTC_EDIT_LAUNCH(1);
  else if (R <= 128) CTC_EDIT_LAUNCH(2);
  else if (R <= 256) CTC_EDIT_LAUNCH(4);
  else if (R <= 512) CTC_EDIT_LAUNCH(8);
  else CTC_EDIT_LAUNCH(16);
#undef CTC_EDIT_LAUNCH
  return hipGetLastError();
}

}  // namespace ctc
