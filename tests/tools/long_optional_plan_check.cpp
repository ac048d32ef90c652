// Stand-alone check of the host plan of the long-form calls with optional wildcards (csrc/ctc_loss_long_plan.h with opt = 1;
// ctc_amd_long_optional_wildcard_loss_grad / _grad_ckpt / _label_posterior): host code only, its own main, in the manner of
// long_loss_plan_check.cpp and long_loss_ckpt_plan_check.cpp.
//   c++ -std=c++17 -I tf_seq2seq_losses_amd/csrc tests/tools/long_optional_plan_check.cpp -o opt_plan_check && ./opt_plan_check
// builds the same with -fsanitize=address,undefined.  It checks
//   1. the regions: the counterpart's plan, offset for offset, and behind it the two further column buffers (16 and, with a gradient,
//      8 bytes per (utterance, block boundary, frame), each rounded to 256); K = 1: the counterpart's size;
//   2. the tiles: with the optional predicate every state that a path can reach -- position i at frame t >= i / 2 of an utterance
//      with L / 2 <= T_b -- lies in a tile that runs, also for T_b < L;
//   3. the dependencies, for small grids and ALL lengths (T_b, L), both workspaces, replaying the launches with the functions the
//      kernels use: everything an alpha tile, a finish kernel, a recompute tile, a beta tile, the row stage or the posterior stage
//      reads -- the two new columns, the row buffer of the block before the last (an end state behind an optional last position)
//      included -- was written on an EARLIER launch by the right tile.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ctc_loss_long_plan.h"

using namespace ctc;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static size_t r256(size_t x) { return (x + 255) / 256 * 256; }

static void check_regions(int kind, int B, int T, int U, int tf) {
  const size_t K = U > 0 ? ((size_t)U + 1023) / 1024 : 1;
  const size_t c16 = r256(16 * (size_t)B * (K - 1) * (size_t)T), c8 = r256(8 * (size_t)B * (K - 1) * (size_t)T);
  for (int ckpt = 0; ckpt < 2; ++ckpt)
    for (int g = 0; g < 2; ++g) {
      LongLossPlan P, Q;
      const bool a = ckpt ? long_loss_ckpt_plan(kind, B, T, U, tf, g, &Q) : long_loss_plan(kind, B, T, U, tf, g, &Q);
      const bool b = ckpt ? long_loss_ckpt_plan(kind, B, T, U, tf, g, &P, 1) : long_loss_plan(kind, B, T, U, tf, g, &P, 1);
      CHECK(a == b, "the optional plan refuses what the counterpart refuses");
      if (!a || !b) continue;
      CHECK(Q.opt == 0 && P.opt == 1 && P.ckpt == Q.ckpt && P.K == Q.K && P.J == Q.J && P.TF == Q.TF && P.launches == Q.launches, "the grid");
      CHECK(P.off_col == Q.off_col && P.off_row == Q.off_row && P.off_stat == Q.off_stat && P.off_logp == Q.off_logp && P.off_flag == Q.off_flag &&
            P.off_colb == Q.off_colb && P.off_rowb == Q.off_rowb && P.off_rows == Q.off_rows, "the counterpart's offsets");
      CHECK(P.off_col2 == Q.total && P.off_colb2 == Q.total + c16 && P.total == Q.total + c16 + (g ? c8 : 0) && P.total % 256 == 0,
            "kind=%d B=%d T=%d U=%d tf=%d ckpt=%d grad=%d: %zu against %zu", kind, B, T, U, tf, ckpt, g, P.total, Q.total);
      if (K == 1) CHECK(P.total == Q.total, "one label block: the counterpart's size");
    }
  LongPostPlan P, Q;
  const bool a = long_post_plan(kind, B, T, U, tf, &Q), b = long_post_plan(kind, B, T, U, tf, &P, 1);
  CHECK(a == b, "the posterior plan");
  if (a && b)
    CHECK(P.total == Q.total + c16 + c8 && P.off_acc == P.L.total && P.off_acc - Q.off_acc == c16 + c8 && P.off_peak - Q.off_peak == c16 + c8,
          "posterior plan kind=%d B=%d T=%d U=%d tf=%d", kind, B, T, U, tf);
}

struct Row {
  int t = -1, k = -1, stamp = -1, state = 0;  // 0: nothing, 1: the chain's state, 2: posteriors, 3: read by the stage behind
};

// one replay: UB label positions per block, tiles of TF frames, a batch of T frames, an utterance of Tb frames and L labels whose
// last position may be optional (the finish kernel and the first beta tiles then read position L - 2 too)
static void replay(int U, int T, int TF, int UB, int Tb, int L, int ckpt) {
  LongLossPlan P;
  const int K = U > 0 ? (U + UB - 1) / UB : 1, J = T > 0 ? (T + TF - 1) / TF : 1;
  P.K = K; P.J = J; P.TF = TF; P.launches = K + J - 1;
  auto act = [&](int k, int j) { return long_loss_tile_active_opt(Tb, L, k, j, TF, UB); };
  // 2. every reachable state lies in a tile that runs
  if (L / 2 <= Tb)
    for (int i = 0; i < (L > 0 ? L : 1); ++i)
      for (int t = i / 2; t < Tb; ++t) CHECK(act(i / UB, t / TF), "state (%d, t=%d) lies in a tile that does not run Tb=%d L=%d TF=%d", i, t, Tb, L, TF);
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < J; ++j) {
      if (!act(k, j)) continue;
      CHECK(k == 0 || act(k - 1, j), "tile (%d,%d) runs and its left neighbour does not Tb=%d L=%d", k, j, Tb, L);
      CHECK((j + 1) * TF >= Tb || act(k, j + 1), "tile (%d,%d) runs and the next in time does not Tb=%d L=%d", k, j, Tb, L);
    }
  const size_t RF = ckpt ? long_loss_ring_frames(K, T, TF) : (size_t)T;
  std::vector<int> stat(J, -1), col(K * J, -1), col2(K * J, -1), colb(K * J, -1), colb2(K * J, -1), rowb(K, -1);
  std::vector<int> ck(K * J, -1);     // ckpt: the checkpoint of tile (k, j); otherwise [k * J]: the row buffer of block k ...
  std::vector<int> row_who(K, -1);    // ... and the tile in time that wrote it last
  std::vector<Row> rows(K * RF);
  std::vector<int> out_rows(T, 0);
  auto row_at = [&](int k, int t) {
    const size_t i = long_loss_row_index(ckpt, 0, K, k, T, t, TF);
    CHECK(i < rows.size(), "saved row (%d, t=%d) at %zu of %zu", k, t, i, rows.size());
    return i < rows.size() ? i : 0;
  };
  auto alpha_reads = [&](int k, int j, int stamp, bool redo, const char *who) {
    if (k > 0 || redo) CHECK(stat[j] >= 0 && stat[j] < stamp, "%s (%d,%d) reads statistics not yet written Tb=%d L=%d", who, k, j, Tb, L);
    if (k > 0) {
      CHECK(col[(k - 1) * J + j] >= 0 && col[(k - 1) * J + j] < stamp, "%s (%d,%d) reads a column not yet written Tb=%d L=%d", who, k, j, Tb, L);
      CHECK(col2[(k - 1) * J + j] >= 0 && col2[(k - 1) * J + j] < stamp, "%s (%d,%d) reads a second column not yet written Tb=%d L=%d", who, k, j, Tb, L);
    }
    if (!long_loss_alpha_fresh_opt(k, j, TF, UB)) {
      CHECK(j > 0 && act(k, j - 1), "%s (%d,%d) reads the row of a tile that did not run Tb=%d L=%d", who, k, j, Tb, L);
      if (ckpt) CHECK(j > 0 && ck[k * J + j - 1] >= 0 && ck[k * J + j - 1] < stamp, "%s (%d,%d) reads a checkpoint not yet written", who, k, j);
      else CHECK(ck[k * J] >= 0 && ck[k * J] < stamp && row_who[k] == j - 1, "%s (%d,%d) reads a row buffer not written by (%d,%d)", who, k, j, k, j - 1);
    } else {
      CHECK(j == 0 || !act(k, j - 1), "%s (%d,%d) starts afresh behind a tile that ran Tb=%d L=%d", who, k, j, Tb, L);
    }
  };
  auto save_rows = [&](int k, int j, int stamp) {
    for (int t = j * TF; t < (j + 1) * TF && t < Tb; ++t) {
      Row &r = rows[row_at(k, t)];
      CHECK(r.state == 0 || r.state == 3, "tile (%d,%d) overwrites the row of t=%d (state %d) before it was read Tb=%d L=%d", k, j, r.t, r.state, Tb, L);
      r.t = t; r.k = k; r.stamp = stamp; r.state = 1;
    }
  };
  int stamp = 0;
  if (T > 0)
    for (int d = 0; d < P.launches; ++d, ++stamp) {
      int k_lo, count;
      long_loss_forward_diagonal(P, d, &k_lo, &count);
      for (int k = k_lo; k < k_lo + count; ++k)
        if (act(k, d - k)) alpha_reads(k, d - k, stamp, false, "alpha");
      for (int k = k_lo; k < k_lo + count; ++k) {  // (writes after every read of the launch)
        const int j = d - k;
        if (!act(k, j)) continue;
        if (k == 0) stat[j] = stamp;
        if (long_loss_has_right(L, k, UB)) col[k * J + j] = col2[k * J + j] = stamp;
        if (ckpt) ck[k * J + j] = stamp;
        else { ck[k * J] = stamp; row_who[k] = j; save_rows(k, j, stamp); }
      }
    }
  // the finish kernel: positions L - 1 and (an optional last position) L - 2, each where its block's last tile in time ran; L = 1:
  // the start state in block 0
  const bool counted = L / 2 <= Tb;
  if (counted && Tb > 0) {
    const int jl = (Tb - 1) / TF;
    for (int i : {L - 1, L - 2, 0}) {
      if (i < 0) continue;
      const int k = i / UB;
      if (!act(k, jl)) {
        for (int j = 0; j < J; ++j) CHECK(!act(k, j), "finish takes log 0 for block %d, of which tile (%d,%d) ran Tb=%d L=%d", k, k, j, Tb, L);
        CHECK(i > 0, "block 0 did not run Tb=%d L=%d", Tb, L);
        continue;
      }
      if (ckpt) CHECK(ck[k * J + jl] >= 0, "finish reads checkpoint (%d,%d), never written Tb=%d L=%d", k, jl, Tb, L);
      else CHECK(ck[k * J] >= 0 && row_who[k] == jl, "finish reads the row buffer of block %d, last written by tile %d Tb=%d L=%d", k, row_who[k], Tb, L);
    }
  }
  ++stamp;
  if (T > 0)
    for (int e = 0; e < P.launches; ++e) {
      int d, k_lo, count;
      long_loss_backward_diagonal(P, e, &d, &k_lo, &count);
      if (ckpt) {  // the recompute tiles
        for (int k = k_lo; k < k_lo + count; ++k)
          if (act(k, d - k)) alpha_reads(k, d - k, stamp, true, "recompute");
        for (int k = k_lo; k < k_lo + count; ++k)
          if (act(k, d - k)) save_rows(k, d - k, stamp);
        ++stamp;
      }
      for (int k = k_lo; k < k_lo + count; ++k) {  // the beta tiles
        const int j = d - k;
        if (!act(k, j) || !counted) continue;
        for (int t = j * TF; t < (j + 1) * TF && t < Tb; ++t) {
          const Row &r = rows[row_at(k, t)];
          CHECK(r.t == t && r.k == k && r.state == 1 && r.stamp < stamp, "beta (%d,%d) reads a row that is not alpha of t=%d Tb=%d L=%d", k, j, t, Tb, L);
        }
        CHECK(stat[j] >= 0, "beta (%d,%d) reads statistics never written", k, j);
        if (k > 0) CHECK(col[(k - 1) * J + j] >= 0 && col2[(k - 1) * J + j] >= 0, "beta (%d,%d) reads an alpha column never written Tb=%d L=%d", k, j, Tb, L);
        if (long_loss_beta_has_right_opt(Tb, L, k, j, TF, UB))
          CHECK(colb[k * J + j] >= 0 && colb[k * J + j] < stamp && colb2[k * J + j] >= 0 && colb2[k * J + j] < stamp,
                "beta (%d,%d) reads a column not yet written Tb=%d L=%d", k, j, Tb, L);
        if (!long_loss_beta_fresh(Tb, j, TF))
          CHECK(rowb[k] >= 0 && rowb[k] < stamp && act(k, j + 1), "beta (%d,%d) reads a row buffer not yet written Tb=%d L=%d", k, j, Tb, L);
      }
      for (int k = k_lo; k < k_lo + count; ++k) {
        const int j = d - k;
        if (!act(k, j) || !counted) continue;
        if (k > 0) colb[(k - 1) * J + j] = colb2[(k - 1) * J + j] = stamp;
        rowb[k] = stamp;
        for (int t = j * TF; t < (j + 1) * TF && t < Tb; ++t) rows[row_at(k, t)].state = 2;
      }
      ++stamp;
      // the row stage or the posterior stage: with checkpoints of time block d, otherwise behind the last launch of all frames
      const int j_lo = ckpt ? d : 0, j_hi = ckpt ? (d < J ? d + 1 : d) : (e == P.launches - 1 ? J : 0);
      for (int j = j_lo; j < j_hi; ++j)
        for (int t = j * TF; t < (j + 1) * TF && t < T; ++t) {
          out_rows[t] += 1;
          if (!counted || t >= Tb) continue;  // zeros
          CHECK(act(0, j) && stat[j] >= 0, "the stage reads statistics never written t=%d Tb=%d L=%d", t, Tb, L);
          for (int k = 0; k < K && (k == 0 || k * UB < L); ++k) {
            if (!act(k, j)) continue;
            Row &r = rows[row_at(k, t)];
            CHECK(r.t == t && r.k == k && r.state == 2 && r.stamp < stamp, "the stage reads a row that is not the posteriors of (%d, t=%d): t=%d state %d Tb=%d L=%d",
                  k, t, r.t, r.state, Tb, L);
            r.state = 3;
          }
        }
      ++stamp;
    }
  for (int t = 0; t < T; ++t) CHECK(out_rows[t] == 1, "output row t=%d written %d times T=%d TF=%d ckpt=%d", t, out_rows[t], T, TF, ckpt);
  if (counted)
    for (const Row &r : rows) CHECK(r.state == 0 || r.state == 3, "a saved row of (%d, t=%d) was never read Tb=%d L=%d ckpt=%d", r.k, r.t, Tb, L, ckpt);
}

int main() {
  const int shapes[][3] = {{0, 0, 0}, {1, 0, 5}, {1, 7, 0}, {2, 5, 4}, {3, 1300, 1024}, {3, 1300, 1025}, {2, 2600, 2100}, {1, 30000, 8192},
                           {1, 180000, 50000}, {3, 30000, 65536}, {1, 100, 3000}, {2, 129, 2049}, {1, 5, 65537}};
  for (const auto &s : shapes)
    for (int kind = 0; kind < 2; ++kind)
      for (int tf : {0, 3, 4, 64, 128, 1300}) check_regions(kind, s[0], s[1], s[2], tf);
  LongLossPlan P;
  CHECK(long_loss_ckpt_plan(0, 1, 30000, 8192, 0, 1, &P) && P.total == (size_t)170923264u, "the counterpart keeps its size: %zu", P.total);
  for (int g = 0; g < 2; ++g) {
    CHECK(long_loss_plan(0, 1, 30000, 8192, 0, g, &P, 1), "plan");
    printf("classic B=1 T=30000 U=8192 grad=%d: %zu bytes per-frame rows", g, P.total);
    CHECK(long_loss_ckpt_plan(0, 1, 30000, 8192, 0, g, &P, 1), "plan");
    printf(", %zu checkpointed; ", P.total);
    CHECK(long_loss_ckpt_plan(0, 1, 180000, 50000, 0, g, &P, 1), "plan");
    printf("the hour (T=180000 U=50000) checkpointed: %zu\n", P.total);
  }

  long replays = 0;
  for (int ckpt = 0; ckpt < 2; ++ckpt) {
    for (int TF : {4, 8, 12})
      for (int U : {0, 1, 8, 9, 16, 17, 30})
        for (int T : {1, 4, 5, 12, 13, 24, 33})
          for (int Tb = 0; Tb <= T; ++Tb)
            for (int L = 0; L <= U; ++L, ++replays) replay(U, T, TF, 8, Tb, L, ckpt);  // (T_b < L included)
    replay(5, 0, 4, 8, 0, 0, ckpt);
    replay(5, 0, 4, 8, 0, 1, ckpt);
    replays += 2;
    // the real block, lengths around every boundary
    for (int TF : {4, 64, 128, 1300})
      for (int Tb : {0, 1, 127, 128, 129, 500, 511, 512, 513, 514, 600, 1023, 1024, 1025, 1200, 2047, 2048, 2049, 2600})
        for (int L : {0, 1, 2, 900, 1023, 1024, 1025, 1026, 1029, 1500, 2047, 2048, 2049, 2050, 2100}) {
          replay(2100, 2600, TF, LONG_UB, Tb, L, ckpt);
          ++replays;
        }
  }
  printf("%ld replays\n", replays);
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
