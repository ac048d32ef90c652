// Stand-alone check of the host plan of the long-form label posteriors (csrc/ctc_loss_long_plan.h, long_post_plan;
// ctc_amd_long_label_posterior): host code only, its own main, in the manner of long_loss_ckpt_plan_check.cpp, which checks the
// forward sweep, the checkpoints and the beta tiles' other inputs of the same schedule.
//   c++ -std=c++17 -I tf_seq2seq_losses_amd/csrc tests/tools/long_post_plan_check.cpp -o post_plan_check && ./post_plan_check
// builds the same with -fsanitize=address,undefined.  It checks
//   1. the regions: the checkpointed gradient's plan, then r256(16 B U) of float64 sums and r256(8 B U) of peaks, 256-byte aligned,
//      and that the last accumulator lies inside its region; the header's worked examples;
//   2. the posterior stage, replaying the backward launches with the functions the kernel uses, for small grids and ALL lengths
//      (T_b, L) and for the real block around every boundary: every ring row that a row wavefront or a position's lane reads holds
//      the posteriors of the right (k, t), written by the beta tile (k, t / TF) on an EARLIER launch and not overwritten since; no
//      ring row is overwritten before the stage of its time block has run; the wavefronts of a launch, mapped as the kernel maps
//      them, cover every (b, t) of the time block and every (b, i) exactly once; every (b, t) is written by exactly one stage; the
//      accumulators of every (b, i) are started before they are read, carried through every stage in descending order of the
//      time blocks, and rounded exactly once, by the last launch; T == 0 still rounds them.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ctc_loss_long_plan.h"

using namespace ctc;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static size_t r256(size_t x) { return (x + 255) / 256 * 256; }

static void check_regions(int kind, int B, int T, int U, int tf) {
  LongPostPlan P;
  LongLossPlan C;
  CHECK(long_post_plan(kind, B, T, U, tf, &P), "kind=%d B=%d T=%d U=%d tf=%d", kind, B, T, U, tf);
  CHECK(long_loss_ckpt_plan(kind, B, T, U, tf, 1, &C), "the checkpointed plan");
  CHECK(P.L.total == C.total && P.L.ckpt == 1 && P.L.off_rows == C.off_rows && P.L.K == C.K && P.L.J == C.J && P.L.TF == C.TF &&
        P.L.launches == C.launches, "the schedule and the workspace of the checkpointed gradient");
  const size_t b = (size_t)B, u = (size_t)U;
  CHECK(P.off_acc == C.total && P.off_acc % 256 == 0, "sums at %zu, expected %zu", P.off_acc, C.total);
  CHECK(P.off_peak == r256(P.off_acc + 16 * b * u) && P.off_peak % 256 == 0, "peaks at %zu", P.off_peak);
  CHECK(P.total == r256(P.off_peak + 8 * b * u), "total %zu", P.total);
  if (B > 0 && U > 0) {
    const size_t at = (size_t)(B - 1) * U + (U - 1);
    CHECK((at + 1) * 16 <= P.off_peak - P.off_acc && (at + 1) * 8 <= P.total - P.off_peak, "the last accumulator");
  }
}

struct RingRow {
  int t = -1, k = -1, stamp = -1;
  int state = 0;  // 0: nothing, 1: the chain's state (recompute tile), 2: posteriors (beta tile)
  int rows_read = 0, lanes_read = 0;  // by the stage of its time block
};

// one replay: B utterances alike, UB label positions per block, tiles of TF frames, a batch of T frames, utterances of Tb frames and
// L labels; per_label: the [B][U] outputs are wanted
static void replay(int B, int U, int T, int TF, int UB, int Tb, int L, bool per_label) {
  LongLossPlan P;
  const int K = U > 0 ? (U + UB - 1) / UB : 1, J = T > 0 ? (T + TF - 1) / TF : 1;
  P.K = K; P.J = J; P.TF = TF; P.launches = K + J - 1;
  const size_t RF = long_loss_ring_frames(K, T, TF), stride = long_loss_row_stride(1, K, T, TF);
  std::vector<RingRow> ring((size_t)B * K * RF);
  std::vector<int> row_written((size_t)B * T, 0);
  // accumulators: 0 nothing, 1 carried in the workspace, 2 rounded; and the time block whose stage touched them last
  std::vector<int> acc((size_t)B * U, 0), acc_block((size_t)B * U, J), acc_final((size_t)B * U, 0);
  const bool feasible = L <= Tb;
  auto act = [&](int k, int j) { return long_loss_tile_active(Tb, L, k, j, TF, UB); };
  auto row_at = [&](int b, int k, int t) {
    const size_t i = long_loss_row_index(1, b, K, k, T, t, TF);
    CHECK(i < ring.size(), "ring row (b=%d, %d, t=%d) at %zu of %zu K=%d T=%d TF=%d", b, k, t, i, ring.size(), K, T, TF);
    CHECK(i == long_loss_row_index(1, b, K, 0, T, t, TF) + (size_t)k * stride, "label blocks lie a stride apart");
    CHECK(i == long_loss_row_index(1, b, K, k, T, t / TF * TF, TF) + (size_t)(t % TF), "the rows of a tile are consecutive");
    return i < ring.size() ? i : 0;
  };
  int stamp = 0, stages = 0;
  // the posterior stage of time block d over nt frames, as loss_long_post_kernel maps its wavefronts
  auto stage = [&](int d, int nt) {
    const size_t row_groups = long_post_row_groups(B, nt), stat_groups = per_label && U > 0 ? long_post_stat_groups(B, U) : 0;
    const int first = d == J - 1, last = d == 0, t0 = d * TF;
    if (row_groups + stat_groups == 0) return;
    ++stages;
    std::vector<int> seen_row((size_t)B * (nt > 0 ? nt : 1), 0), seen_pos((size_t)B * (U > 0 ? U : 1), 0);
    for (size_t g = 0; g < row_groups + stat_groups; ++g)
      for (int wv = 0; wv < LONG_POST_WAVES; ++wv) {
        if (g < row_groups) {
          const long rowi = (long)g * LONG_POST_WAVES + wv;
          if (rowi >= (long)B * nt) continue;
          const int b = (int)(rowi / nt), t = t0 + (int)(rowi % nt);
          CHECK(t >= 0 && t < T && t / TF == d, "row wavefront at t=%d outside time block %d", t, d);
          seen_row[(size_t)b * nt + (t - t0)] += 1;
          row_written[(size_t)b * T + t] += 1;
          if (!(t < Tb && feasible)) continue;  // zeros
          CHECK(act(0, d), "a live frame whose tile (0, %d) did not run t=%d Tb=%d L=%d", d, t, Tb, L);
          for (int k = 0; k < K; ++k) {
            if (!((k == 0 || k * UB < L) && act(k, d))) continue;  // zeros
            RingRow &r = ring[row_at(b, k, t)];
            CHECK(r.t == t && r.k == k && r.state == 2 && r.stamp < stamp, "a row wavefront reads a row that is not the posteriors of (%d, t=%d): t=%d k=%d state %d Tb=%d L=%d TF=%d",
                  k, t, r.t, r.k, r.state, Tb, L, TF);
            r.rows_read += 1;
          }
        } else {
          const int groups = (U + 63) / 64;
          const long wi = (long)(g - row_groups) * LONG_POST_WAVES + wv;
          if (wi >= (long)B * groups) continue;
          for (int lane = 0; lane < 64; ++lane) {
            const int b = (int)(wi / groups), i = (int)(wi % groups) * 64 + lane;
            if (i >= U) continue;
            const size_t at = (size_t)b * U + i;
            CHECK(at < acc.size(), "accumulator %zu of %zu", at, acc.size());
            seen_pos[at] += 1;
            if (!first) CHECK(acc[at] == 1 && acc_block[at] == d + 1, "the accumulators of (b=%d, i=%d) are read in stage %d before stage %d stored them (state %d, last block %d)",
                              b, i, d, d + 1, acc[at], acc_block[at]);
            else CHECK(acc[at] == 0, "the accumulators of (b=%d, i=%d) are started twice", b, i);
            const int k = i / UB;
            // (the lanes of a label block read the same rows at their own slots: its first, its last and the last label witness them)
            const bool witness = i % UB == 0 || i % UB == UB - 1 || i == L - 1;
            if (witness && feasible && i < L && nt > 0 && act(k, d)) {
              const int t_hi = Tb - t0 < nt ? Tb : t0 + nt;
              CHECK(t_hi > t0, "an active tile without a frame");
              for (int t = t_hi - 1; t >= t0; --t) {
                RingRow &r = ring[row_at(b, k, t)];
                CHECK(r.t == t && r.k == k && r.state == 2 && r.stamp < stamp, "position %d reads a row that is not the posteriors of (%d, t=%d): t=%d state %d Tb=%d L=%d TF=%d",
                      i, k, t, r.t, r.state, Tb, L, TF);
                r.lanes_read += 1;
              }
            }
            acc_block[at] = d;
            if (last) { acc[at] = 2; acc_final[at] += 1; } else { acc[at] = 1; }
          }
        }
      }
    for (size_t q = 0; q < (size_t)B * nt; ++q) CHECK(seen_row[q] == 1, "row %zu of time block %d covered %d times", q, d, seen_row[q]);
    if (stat_groups)
      for (size_t q = 0; q < (size_t)B * U; ++q) CHECK(seen_pos[q] == 1, "position %zu covered %d times in stage %d", q, seen_pos[q], d);
    ++stamp;
  };

  if (T == 0) {
    stage(0, 0);
  } else {
    for (int e = 0; e < P.launches; ++e) {
      int d, k_lo, count;
      long_loss_backward_diagonal(P, e, &d, &k_lo, &count);
      for (int b = 0; b < B; ++b)  // the recompute tiles
        for (int k = k_lo; k < k_lo + count; ++k) {
          const int j = d - k;
          if (!act(k, j)) continue;
          for (int t = j * TF; t < (j + 1) * TF && t < Tb; ++t) {
            RingRow &r = ring[row_at(b, k, t)];
            // what is overwritten has been through the stage of its time block (r.t / TF > d: that stage ran on an earlier launch)
            CHECK(r.state == 0 || (r.state == 2 && r.t / TF > d && r.t / TF < J), "recompute (%d,%d) overwrites the row of t=%d (state %d) before its stage Tb=%d L=%d K=%d J=%d TF=%d",
                  k, j, r.t, r.state, Tb, L, K, J, TF);
            r = RingRow();
            r.t = t; r.k = k; r.stamp = stamp; r.state = 1;
          }
        }
      ++stamp;
      for (int b = 0; b < B; ++b)  // the beta tiles
        for (int k = k_lo; k < k_lo + count; ++k) {
          const int j = d - k;
          if (!act(k, j)) continue;
          for (int t = j * TF; t < (j + 1) * TF && t < Tb; ++t) {
            RingRow &r = ring[row_at(b, k, t)];
            CHECK(r.t == t && r.k == k && r.state == 1 && r.stamp < stamp, "beta (%d,%d) reads a row that is not alpha of t=%d", k, j, t);
            r.state = 2; r.stamp = stamp;
          }
        }
      ++stamp;
      if (d < J) stage(d, T - d * TF < TF ? T - d * TF : TF);
    }
  }
  for (size_t q = 0; q < row_written.size(); ++q) CHECK(row_written[q] == 1, "row %zu written %d times T=%d TF=%d", q, row_written[q], T, TF);
  if (per_label)
    for (size_t q = 0; q < acc.size(); ++q) CHECK(acc[q] == 2 && acc_final[q] == 1 && acc_block[q] == 0, "position %zu rounded %d times (state %d)", q, acc_final[q], acc[q]);
  CHECK(stages == (T > 0 ? J : (per_label && U > 0 && B > 0 ? 1 : 0)), "%d stages for J=%d T=%d", stages, J, T);
  // every row of posteriors of a label block that has labels was read by the stage of its time block, by a row wavefront and by lanes
  for (const RingRow &r : ring)
    if (r.state == 2 && (r.k == 0 || r.k * UB < L)) {
      CHECK(r.rows_read == 1, "the posteriors of (%d, t=%d) were read by %d row wavefronts Tb=%d L=%d", r.k, r.t, r.rows_read, Tb, L);
      if (per_label && L > 0) CHECK(r.lanes_read >= 1, "the posteriors of (%d, t=%d) were read by no position Tb=%d L=%d", r.k, r.t, Tb, L);
    }
}

int main() {
  // 1. regions
  const int shapes[][3] = {{0, 0, 0}, {1, 0, 5}, {1, 7, 0}, {2, 5, 4}, {3, 1300, 1025}, {2, 2600, 2100}, {1, 30000, 8192}, {8, 30000, 8192},
                           {1, 180000, 50000}, {3, 30000, 65536}, {8, 180000, 65536}, {1, 100, 3000}, {2, 129, 2049}};
  for (const auto &s : shapes)
    for (int kind = 0; kind < 2; ++kind)
      for (int tf : {0, 4, 64, 128, 1000, 1300}) check_regions(kind, s[0], s[1], s[2], tf);
  LongPostPlan P;
  CHECK(long_post_plan(0, 1, 30000, 8192, 0, &P) && P.total == (size_t)171119872u, "B=1 T=30000 U=8192 classic: %zu bytes", P.total);
  CHECK(long_post_plan(0, 1, 180000, 50000, 0, &P) && P.total == (size_t)6386400512ull, "an hour of audio: %zu bytes", P.total);
  printf("classic B=1 T=30000 U=8192: %zu bytes; ", (long_post_plan(0, 1, 30000, 8192, 0, &P), P.total));
  printf("simplified: %zu bytes; ", (long_post_plan(1, 1, 30000, 8192, 0, &P), P.total));
  printf("the hour, classic: %zu bytes, simplified: ", (long_post_plan(0, 1, 180000, 50000, 0, &P), P.total));
  printf("%zu bytes\n", (long_post_plan(1, 1, 180000, 50000, 0, &P), P.total));
  // what the plan refuses: what long_loss_ckpt_plan refuses with a gradient, and a stage of more than 2^31 - 1 workgroups
  CHECK(!long_post_plan(2, 1, 5, 4, 0, &P) && !long_post_plan(0, 1, 5, 4, 3, &P) && !long_post_plan(0, 1, 5, 65537, 0, &P) &&
        !long_post_plan(0, -1, 5, 4, 0, &P) && !long_post_plan(0, 1 << 20, 1 << 14, 4, 0, &P), "refusals");
  LongLossPlan C;  // (2^20 * 1028 row groups and 2^30 groups of positions: each fits a grid, their sum does not)
  CHECK(!long_post_plan(0, 1 << 22, 1028, 65536, 1028, &P) && long_loss_ckpt_plan(0, 1 << 22, 1028, 65536, 1028, 1, &C) &&
        long_post_plan(0, 1 << 22, 1020, 65536, 1020, &P), "the posterior stage's grid");

  // 2. small grids, all lengths: blocks of UB = 8 positions, tiles of 4, 8 and 12 frames (J < K, J == K, J > K: the ring wraps)
  long replays = 0;
  for (int TF : {4, 8, 12})
    for (int U : {0, 1, 8, 9, 16, 17, 30})
      for (int T : {1, 4, 5, 12, 13, 24, 33, 67})
        for (int Tb = 0; Tb <= T; ++Tb)
          for (int L = 0; L <= U; ++L, ++replays) replay(2, U, T, TF, 8, Tb, L, (Tb + L) % 3 != 0);
  for (int U : {0, 5, 70}) {  // T == 0
    replay(3, U, 0, 4, 8, 0, 0, true);
    replay(3, U, 0, 4, 8, 0, U, true);
    replay(3, U, 0, 4, 8, 0, 0, false);
    replays += 3;
  }
  // the real block, lengths around every boundary (B = 3: the row wavefronts of a workgroup straddle utterances)
  for (int TF : {4, 64, 128, 1300})
    for (int Tb : {0, 1, 127, 128, 129, 1023, 1024, 1025, 1200, 2047, 2048, 2049, 2300, 2600})
      for (int L : {0, 1, 900, 1023, 1024, 1025, 1500, 2047, 2048, 2049, 2100}) {
        replay(3, 2100, 2600, TF, LONG_UB, Tb, L, true);
        ++replays;
      }
  printf("%ld replays\n", replays);
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
