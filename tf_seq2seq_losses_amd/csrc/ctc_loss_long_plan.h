// Host-side plan of the tiled CTC loss and gradient (ctc_loss_long.hip, ctc_amd_long_wildcard_loss_grad): the tile grid of
// ctc_align_long_plan.h, the forward and backward launch schedules, the one predicate that says which tiles run, and the workspace
// offsets.  Plain C++ with no HIP in it, so that tests/tools/long_loss_plan_check.cpp can run it under the host sanitizers; the
// predicates are compiled for the device too (the kernels call the same functions).  Every byte count is a size_t: the saved rows
// take 8 * B * K * T * (S * 1024 + 2) bytes and pass 2^32 at realistic sizes.
#pragma once
#include <stddef.h>

#include "ctc_align_long_plan.h"

#if defined(__HIPCC__)
#define CTC_LL_HD __host__ __device__ inline
#else
#define CTC_LL_HD inline
#endif

namespace ctc {

// doubles of a saved row of one (utterance, label block, frame): per position the pair (O, C) (classic) or S (simplified), then the
// start state (block 0 only) and one double of padding -- the row of ctc_wild_loss.hip at UP = LONG_UB
constexpr int long_loss_row_doubles(int kind) { return (kind == 0 ? 2 : 1) * LONG_UB + 2; }

// ---- which tiles run ----
// Tile (k, j) holds the label positions k * UB .. k * UB + UB - 1 and the frames j * TF .. j * TF + TF - 1 of an utterance of Tb
// frames and L labels (L <= U: an utterance with more labels runs no tile at all).  A tile that does not run writes nothing, and
// nothing of it is ever read: every reader below asks the same function.
//   L > Tb                       infeasible by the count (every position takes a frame of its own): no tile runs
//   j * TF >= Tb                 beyond the frames
//   k > 0 and k * UB >= L        beyond the labels (block 0 runs for an empty transcript too: the start state lives there)
//   j * TF + TF - 1 < k * UB     alpha of position i is log 0 before frame i: the whole tile is, and so are its posteriors
// The beta sweep needs nothing more: a tile that the last test drops would hand beta to paths that no alpha reaches, whose
// posteriors are exactly 0 whatever beta is, so its left neighbour takes log 0 in its place.
CTC_LL_HD bool long_loss_tile_active(int Tb, int L, int k, int j, int TF, int UB = LONG_UB) {
  if (L > Tb) return false;
  if ((long long)j * TF >= Tb) return false;
  if (k > 0 && (long long)k * UB >= L) return false;
  if ((long long)j * TF + TF - 1 < (long long)k * UB) return false;
  return true;
}
// Optional wildcards: a position may take no frame, but no two such positions are adjacent, so position i
// is log 0 before frame i / 2 and L positions need L / 2 frames: the first and the last test on those bounds.  A tile that runs
// over states that nothing reaches carries log 0 and changes no bit; what is infeasible falls out of the lattice.
CTC_LL_HD bool long_loss_tile_active_opt(int Tb, int L, int k, int j, int TF, int UB = LONG_UB) {
  if (L / 2 > Tb) return false;
  if ((long long)j * TF >= Tb) return false;
  if (k > 0 && (long long)k * UB >= L) return false;
  if ((long long)j * TF + TF - 1 < (long long)k * UB / 2) return false;
  return true;
}
// (all four for a tile that runs)
// alpha: the block's first tile starts from log 0 (block 0, tile 0: from the start state); every other reads the row buffer
CTC_LL_HD bool long_loss_alpha_fresh(int k, int j, int TF, int UB = LONG_UB) { return (long long)j * TF <= (long long)k * UB; }
// (optional wildcards: the tile before it in time did not run, by the last test of long_loss_tile_active_opt)
CTC_LL_HD bool long_loss_alpha_fresh_opt(int k, int j, int TF, int UB = LONG_UB) { return (long long)j * TF <= (long long)k * UB / 2; }
// alpha: block k + 1 has labels, so this tile stores the column (its last position before every frame); the tile to the right then
// runs for every frame range in which it could read it
CTC_LL_HD bool long_loss_has_right(int L, int k, int UB = LONG_UB) { return (long long)(k + 1) * UB < L; }
// beta: the block's last tile in time starts from the end state; every other reads the beta row buffer
CTC_LL_HD bool long_loss_beta_fresh(int Tb, int j, int TF) { return (long long)(j + 1) * TF >= Tb; }
// beta: the tile to the right ran on an earlier launch and stored its column (else: log 0)
CTC_LL_HD bool long_loss_beta_has_right(int Tb, int L, int k, int j, int TF, int UB = LONG_UB) {
  return long_loss_has_right(L, k, UB) && long_loss_tile_active(Tb, L, k + 1, j, TF, UB);
}
CTC_LL_HD bool long_loss_beta_has_right_opt(int Tb, int L, int k, int j, int TF, int UB = LONG_UB) {
  return long_loss_has_right(L, k, UB) && long_loss_tile_active_opt(Tb, L, k + 1, j, TF, UB);
}

// ---- where things live ----
// The checkpointed gradient (ctc_amd_long_wildcard_loss_grad_ckpt) keeps the chain row that leaves tile (k, j) in a slot of its own,
// [b][k][j] of [B][K][Jc], Jc = max(J, 1) time blocks, and the saved rows of a tile only while its time block is in flight: a ring
// of R = min(K, Jc) time blocks per (utterance, label block).
CTC_LL_HD int long_loss_ckpt_cols(int T, int TF) { return T > 0 ? (int)(((long long)T + TF - 1) / TF) : 1; }
CTC_LL_HD int long_loss_ring_cols(int K, int T, int TF) {
  const int Jc = long_loss_ckpt_cols(T, TF);
  return K < Jc ? K : Jc;
}
// frames of the ring of one (utterance, label block): R * TF, and no more than T (R == Jc: every time block has its own slot, the
// last one is T - (Jc - 1) * TF frames long, and the slots are the per-frame rows themselves)
CTC_LL_HD size_t long_loss_ring_frames(int K, int T, int TF) {
  const size_t rt = (size_t)long_loss_ring_cols(K, T, TF) * (size_t)TF;
  return rt < (size_t)T ? rt : (size_t)T;
}
// index of the checkpoint of tile (k, j) of utterance b, in chain states of LONG_ROW_DOUBLES doubles
CTC_LL_HD size_t long_loss_ckpt_index(int b, int K, int k, int T, int TF, int j) {
  return ((size_t)b * K + k) * (size_t)long_loss_ckpt_cols(T, TF) + (size_t)j;
}
// index of the saved row of (b, k, t), in rows of long_loss_row_doubles(kind) doubles: the one function that the alpha tile that
// saves rows, the beta tile, the row stage and the plan checkers ask.  ckpt == 0: [B][K][T].  ckpt != 0: the ring
// [B][K][(t / TF) mod R][t mod TF], whose time blocks lie TF rows apart (the rows of one tile are consecutive in both).
// long_loss_row_stride: the rows between one label block and the next, index(k) = index(0) + k * stride (the row stage walks that).
CTC_LL_HD size_t long_loss_row_stride(int ckpt, int K, int T, int TF) { return ckpt ? long_loss_ring_frames(K, T, TF) : (size_t)T; }
CTC_LL_HD size_t long_loss_row_index(int ckpt, int b, int K, int k, int T, int t, int TF) {
  if (!ckpt) return ((size_t)b * K + k) * (size_t)T + (size_t)t;
  const int j = t / TF, R = long_loss_ring_cols(K, T, TF);
  return ((size_t)b * K + k) * long_loss_ring_frames(K, T, TF) + (size_t)(j % R) * TF + (size_t)(t - j * TF);
}

struct LongLossPlan {
  int kind, B, T, U, want_grad;
  int K, J, TF;   // label blocks, time blocks, frames per tile
  int launches;   // K + J - 1 anti-diagonals of tiles per sweep (none when T == 0)
  int ckpt;       // 1: the checkpointed layout (long_loss_ckpt_plan with a gradient); off_row is then [B][K][Jc], off_rows the ring
  size_t off_col, off_row, off_stat, off_logp, off_flag;  // both paths
  size_t off_colb, off_rowb, off_rows;                    // the gradient's (want_grad == 0: all equal to total)
  int opt;                     // 1: optional wildcards, the two further column buffers behind everything else
  size_t off_col2, off_colb2;  // (opt == 0: unused)
  size_t total;
};

// Optional wildcards: a skip reaches two positions back, so a second alpha column (position k * UB - 2
// before every frame) and, with a gradient, a second beta column (the worth of entering position (k + 1) * UB + 1 with the frame)
// cross a block boundary.  They lie behind the plan as it was: every other offset is the counterpart's.
inline void long_loss_plan_add_optional(LongLossPlan *P) {
  const size_t b = (size_t)P->B, t = (size_t)P->T, k = (size_t)P->K;
  size_t o = P->total;
  P->opt = 1;
  P->off_col2 = o;  o = long_r256(o + b * (k - 1) * t * 16);  // [B][K - 1][T] pairs (O, C) of float64
  P->off_colb2 = o;
  if (P->want_grad) o = long_r256(o + b * (k - 1) * t * 8);   // [B][K - 1][T] float64
  P->total = o;
}

// false: what long_plan refuses (frames_per_tile, sizes, the tile grid), or, with a gradient, a row stage of more than 2^31 - 1
// workgroups (four rows (b, t) each)
inline bool long_loss_plan(int kind, int B, int T, int U, int frames_per_tile, int want_grad, LongLossPlan *out, int opt = 0) {
  LongPlan A;
  if (kind < 0 || kind > 1 || !long_plan(B, T, U, frames_per_tile, &A)) return false;
  if (want_grad && ((long long)B * T + 3) / 4 > 0x7fffffffLL) return false;
  LongLossPlan P;
  P.kind = kind; P.B = B; P.T = T; P.U = U; P.want_grad = want_grad ? 1 : 0;
  P.K = A.K; P.J = A.J; P.TF = A.TF; P.launches = A.launches; P.ckpt = 0;
  const size_t b = (size_t)B, t = (size_t)T, k = (size_t)P.K;
  size_t o = 0;
  P.off_col = o;  o = long_r256(o + b * (k - 1) * t * 16);          // alpha columns: [B][K - 1][T] pairs (O, C) of float64
  P.off_row = o;  o = long_r256(o + b * k * LONG_ROW_DOUBLES * 8);  // alpha row buffers: [B][K] chain states
  P.off_stat = o; o = long_r256(o + b * t * 16);                    // row statistics: [B][T] x[blank], max, log2 sum exp, 0 (float32)
  P.off_logp = o; o = long_r256(o + b * 8);                         // log2 Z: [B] float64
  P.off_flag = o; o = long_r256(o + b * 4);                         // feasible: [B] int32
  P.off_colb = o;
  if (want_grad) o = long_r256(o + b * (k - 1) * t * 8);            // beta columns: [B][K - 1][T] float64
  P.off_rowb = o;
  if (want_grad) o = long_r256(o + b * k * LONG_ROW_DOUBLES * 8);   // beta row buffers: [B][K] chain states
  P.off_rows = o;
  if (want_grad) o = long_r256(o + b * k * t * (size_t)long_loss_row_doubles(kind) * 8);  // saved rows: [B][K][T][S * 1024 + 2] float64
  P.total = o;
  P.opt = 0; P.off_col2 = P.off_colb2 = o;
  if (opt) long_loss_plan_add_optional(&P);
  *out = P;
  return true;
}

// The checkpointed call's plan.  Without a gradient it is long_loss_plan's (the call runs the existing forward).  With one, two terms
// differ: the alpha row buffers become the checkpoints [B][K][Jc], and the saved rows become the ring [B][K][min(R * TF, T)] rows,
// never more than the T rows it replaces.  Refuses what long_loss_plan refuses.
inline bool long_loss_ckpt_plan(int kind, int B, int T, int U, int frames_per_tile, int want_grad, LongLossPlan *out, int opt = 0) {
  LongLossPlan P;
  if (!long_loss_plan(kind, B, T, U, frames_per_tile, want_grad, &P, want_grad ? 0 : opt)) return false;
  if (!want_grad) { *out = P; return true; }
  P.ckpt = 1;
  const size_t b = (size_t)P.B, t = (size_t)P.T, k = (size_t)P.K;
  size_t o = P.off_row;  // (the alpha columns before it: as they are)
  o = long_r256(o + b * k * (size_t)long_loss_ckpt_cols(P.T, P.TF) * LONG_ROW_DOUBLES * 8);  // alpha checkpoints: [B][K][Jc] chain states
  P.off_stat = o; o = long_r256(o + b * t * 16);
  P.off_logp = o; o = long_r256(o + b * 8);
  P.off_flag = o; o = long_r256(o + b * 4);
  P.off_colb = o; o = long_r256(o + b * (k - 1) * t * 8);
  P.off_rowb = o; o = long_r256(o + b * k * LONG_ROW_DOUBLES * 8);
  P.off_rows = o; o = long_r256(o + b * k * long_loss_ring_frames(P.K, P.T, P.TF) * (size_t)long_loss_row_doubles(kind) * 8);  // the ring
  P.total = o;
  P.off_col2 = P.off_colb2 = o;
  if (opt) long_loss_plan_add_optional(&P);
  *out = P;
  return true;
}

// The plan of the long-form label posteriors (ctc_amd_long_label_posterior): the checkpointed gradient's,
// schedule and all, with the posterior stage in the row stage's place, and behind it what that stage carries from time block to time
// block per (utterance, label position): the float64 sums (sum p, sum t p) and the running peak with its frame.
struct LongPostPlan {
  LongLossPlan L;            // long_loss_ckpt_plan(want_grad = 1)
  size_t off_acc, off_peak;  // [B][U] pairs of float64; [B][U] pairs (float32 peak, int32 frame)
  size_t total;
};
// wavefronts of one launch of the posterior stage: first one per row (b, t) of a time block of nt frames, then one per (utterance,
// 64 label positions); LONG_POST_WAVES to a workgroup, each part rounded up to whole workgroups
constexpr int LONG_POST_WAVES = 4;
CTC_LL_HD size_t long_post_row_groups(int B, int nt) { return ((size_t)B * (size_t)nt + LONG_POST_WAVES - 1) / LONG_POST_WAVES; }
CTC_LL_HD size_t long_post_stat_groups(int B, int U) { return ((size_t)B * (((size_t)U + 63) / 64) + LONG_POST_WAVES - 1) / LONG_POST_WAVES; }
// false: what long_loss_ckpt_plan refuses with a gradient, or a posterior stage of more than 2^31 - 1 workgroups
inline bool long_post_plan(int kind, int B, int T, int U, int frames_per_tile, LongPostPlan *out, int opt = 0) {
  LongPostPlan P;
  if (!long_loss_ckpt_plan(kind, B, T, U, frames_per_tile, 1, &P.L, opt)) return false;
  if (long_post_row_groups(B, T < P.L.TF ? T : P.L.TF) + long_post_stat_groups(B, U) > 2147483647u) return false;
  size_t o = P.L.total;
  P.off_acc = o;  o = long_r256(o + (size_t)B * (size_t)U * 16);
  P.off_peak = o; o = long_r256(o + (size_t)B * (size_t)U * 8);
  P.total = o;
  *out = P;
  return true;
}

// forward launch d of 0 .. launches - 1 runs the tiles (k, d - k), k = *k_lo .. *k_lo + *count - 1, of every utterance: tile (k, j)
// after (k - 1, j), (k, j - 1) and (0, j)
inline void long_loss_forward_diagonal(const LongLossPlan &P, int d, int *k_lo, int *count) {
  const int lo = d - (P.J - 1) > 0 ? d - (P.J - 1) : 0, hi = d < P.K - 1 ? d : P.K - 1;
  *k_lo = lo;
  *count = hi - lo + 1;
}
// backward launch e of 0 .. launches - 1 runs the tiles of the forward diagonal launches - 1 - e: tile (k, j) after (k + 1, j) and
// (k, j + 1)
inline void long_loss_backward_diagonal(const LongLossPlan &P, int e, int *d, int *k_lo, int *count) {
  *d = P.launches - 1 - e;
  long_loss_forward_diagonal(P, *d, k_lo, count);
}

}  // namespace ctc
