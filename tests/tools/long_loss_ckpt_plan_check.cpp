// Stand-alone check of the host plan of the checkpointed long-form CTC gradient (csrc/ctc_loss_long_plan.h, long_loss_ckpt_plan;
// ctc_amd_long_wildcard_loss_grad_ckpt): host code only, its own main, in the manner of long_loss_plan_check.cpp.
//   c++ -std=c++17 -I tf_seq2seq_losses_amd/csrc tests/tools/long_loss_ckpt_plan_check.cpp -o ckpt_plan_check && ./ckpt_plan_check
// builds the same with -fsanitize=address,undefined.  It checks
//   1. the regions: monotone offsets, 256-byte aligned, sizes as the header of include/ctc_amd.h states them; without a gradient the
//      plan is long_loss_plan's; the ring never exceeds the per-frame rows it replaces; the hour of audio;
//   2. the addressing: checkpoints and ring rows stay inside their regions, the rows of a tile are consecutive, the label blocks lie
//      long_loss_row_stride apart;
//   3. the dependencies, for small grids and ALL lengths (T_b, L), replaying the launches with the functions the kernels use:
//      everything a forward tile, the finish kernel, a recompute tile, a beta tile or a row-stage column reads was written on an
//      EARLIER launch by the right (k, j) -- for a ring row: holds the right frame in the right state --, no ring row is overwritten
//      before the row stage of its time block has read it, and the row stage covers every (b, t) exactly once.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ctc_loss_long_plan.h"

using namespace ctc;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static size_t r256(size_t x) { return (x + 255) / 256 * 256; }

static void terms_of(int kind, int B, int T, int U, int tf, size_t sizes[8]) {
  const size_t TF = tf ? tf : 128;
  const size_t b = (size_t)B, t = (size_t)T, k = (size_t)(U > 0 ? (U + 1023) / 1024 : 1), S = kind == 0 ? 2 : 1;
  const size_t J = T > 0 ? (t + TF - 1) / TF : 1, R = k < J ? k : J, ring = R * TF < t ? R * TF : t;
  const size_t s[8] = {16 * b * (k - 1) * t, 8 * b * k * J * 2056, 16 * b * t, 8 * b, 4 * b, 8 * b * (k - 1) * t, 8 * b * k * 2056,
                       8 * b * k * ring * (S * 1024 + 2)};
  for (int i = 0; i < 8; ++i) sizes[i] = s[i];
}

static void check_regions(int kind, int B, int T, int U, int tf) {
  LongLossPlan P, Q, F;
  CHECK(long_loss_ckpt_plan(kind, B, T, U, tf, 1, &P), "kind=%d B=%d T=%d U=%d tf=%d", kind, B, T, U, tf);
  CHECK(long_loss_plan(kind, B, T, U, tf, 1, &Q) && long_loss_plan(kind, B, T, U, tf, 0, &F), "the existing plans");
  size_t sizes[8];
  terms_of(kind, B, T, U, tf, sizes);
  const size_t offs[8] = {P.off_col, P.off_row, P.off_stat, P.off_logp, P.off_flag, P.off_colb, P.off_rowb, P.off_rows};
  size_t o = 0;
  for (int i = 0; i < 8; ++i) {
    CHECK(offs[i] == o && offs[i] % 256 == 0, "region %d at %zu, expected %zu (B=%d T=%d U=%d tf=%d)", i, offs[i], o, B, T, U, tf);
    o = r256(o + sizes[i]);
  }
  CHECK(P.total == o && P.ckpt == 1, "total %zu, expected %zu", P.total, o);
  CHECK(P.K == Q.K && P.J == Q.J && P.TF == Q.TF && P.launches == Q.launches, "the grid is the existing call's");
  CHECK(P.total - P.off_rows <= Q.total - Q.off_rows, "the ring (%zu) exceeds the per-frame rows (%zu) B=%d T=%d U=%d tf=%d",
        P.total - P.off_rows, Q.total - Q.off_rows, B, T, U, tf);
  // the regions hold what the addressing reaches
  if (B > 0 && T > 0) {
    const size_t SRD = (size_t)long_loss_row_doubles(kind);
    CHECK((long_loss_ckpt_index(B - 1, P.K, P.K - 1, T, P.TF, P.J - 1) + 1) * LONG_ROW_DOUBLES * 8 <= P.off_stat - P.off_row, "last checkpoint");
    size_t hi = 0;
    for (int t = T - 1; t >= 0 && t >= T - 2 * P.TF * P.K; --t) {
      const size_t x = long_loss_row_index(1, B - 1, P.K, P.K - 1, T, t, P.TF);
      hi = x > hi ? x : hi;
    }
    CHECK((hi + 1) * SRD * 8 <= P.total - P.off_rows, "last ring row %zu B=%d T=%d U=%d tf=%d", hi, B, T, U, tf);
  }
  // without a gradient: the existing forward-only plan
  LongLossPlan N;
  CHECK(long_loss_ckpt_plan(kind, B, T, U, tf, 0, &N) && N.total == F.total && N.ckpt == 0 && N.off_row == F.off_row && N.off_rows == F.total,
        "forward only");
}

static void print_terms(const char *what, int kind, int B, int T, int U, int tf) {
  LongLossPlan P, Q;
  size_t s[8];
  terms_of(kind, B, T, U, tf, s);
  if (!long_loss_ckpt_plan(kind, B, T, U, tf, 1, &P) || !long_loss_plan(kind, B, T, U, tf, 1, &Q)) { CHECK(false, "plan"); return; }
  printf("%s B=%d T=%d U=%d tf=%d (K=%d J=%d R=%d): alpha columns %zu, checkpoints %zu, statistics %zu, log2 Z %zu, feasible %zu, "
         "beta columns %zu, beta rows %zu, ring %zu; %zu bytes checkpointed, %zu existing (%.1f x)\n",
         what, B, T, U, P.TF, P.K, P.J, long_loss_ring_cols(P.K, T, P.TF), s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], P.total, Q.total,
         (double)Q.total / (double)P.total);
}

struct RingRow {
  int t = -1, k = -1, stamp = -1;
  int state = 0;  // 0: nothing, 1: the chain's state (recompute tile), 2: posteriors (beta tile), 3: read by the row stage
};

// one replay: UB label positions per block, tiles of TF frames, a batch of T frames, an utterance of Tb frames and L labels
static void replay(int U, int T, int TF, int UB, int Tb, int L) {
  LongLossPlan P;
  const int K = U > 0 ? (U + UB - 1) / UB : 1, J = T > 0 ? (T + TF - 1) / TF : 1;
  P.K = K; P.J = J; P.TF = TF; P.launches = K + J - 1;
  const int Jc = long_loss_ckpt_cols(T, TF), R = long_loss_ring_cols(K, T, TF);
  const size_t RF = long_loss_ring_frames(K, T, TF), stride = long_loss_row_stride(1, K, T, TF);
  CHECK(Jc == J && R == (K < J ? K : J) && RF <= (size_t)T && stride == RF, "geometry K=%d J=%d", K, J);
  std::vector<int> stat(J, -1), col(K * J, -1), colb(K * J, -1), rowb(K, -1);
  std::vector<int> ck(K * Jc, -1), ck_who(K * Jc, -1);  // launch stamp and writer (k * J + j) of every checkpoint
  std::vector<RingRow> ring(K * RF);
  std::vector<int> seen(K * J, 0), grad_rows(T, 0);
  const bool counted = L <= Tb;
  auto act = [&](int k, int j) { return long_loss_tile_active(Tb, L, k, j, TF, UB); };
  auto ck_at = [&](int k, int j) {
    const size_t i = long_loss_ckpt_index(0, K, k, T, TF, j);
    CHECK(i < ck.size(), "checkpoint (%d,%d) at %zu of %zu", k, j, i, ck.size());
    return i < ck.size() ? i : 0;
  };
  auto row_at = [&](int k, int t) {
    const size_t i = long_loss_row_index(1, 0, K, k, T, t, TF);
    CHECK(i < ring.size(), "ring row (%d, t=%d) at %zu of %zu K=%d T=%d TF=%d", k, t, i, ring.size(), K, T, TF);
    CHECK(i == long_loss_row_index(1, 0, K, 0, T, t, TF) + (size_t)k * stride, "label blocks lie a stride apart");
    CHECK(i == long_loss_row_index(1, 0, K, k, T, t / TF * TF, TF) + (size_t)(t % TF), "the rows of a tile are consecutive");
    return i < ring.size() ? i : 0;
  };
  auto alpha_reads = [&](int k, int j, int stamp, const char *who) {
    if (k > 0 || who[0] == 'r') CHECK(stat[j] >= 0 && stat[j] < stamp, "%s (%d,%d) reads statistics not yet written Tb=%d L=%d", who, k, j, Tb, L);
    if (k > 0) CHECK(col[(k - 1) * J + j] >= 0 && col[(k - 1) * J + j] < stamp, "%s (%d,%d) reads a column not yet written Tb=%d L=%d", who, k, j, Tb, L);
    if (!long_loss_alpha_fresh(k, j, TF, UB)) {
      const size_t i = j > 0 ? ck_at(k, j - 1) : 0;
      CHECK(j > 0 && ck[i] >= 0 && ck[i] < stamp && ck_who[i] == k * J + j - 1, "%s (%d,%d) reads a checkpoint not written by (%d,%d) Tb=%d L=%d",
            who, k, j, k, j - 1, Tb, L);
    } else {
      CHECK(j == 0 || !act(k, j - 1), "%s (%d,%d) starts afresh behind a tile that ran Tb=%d L=%d", who, k, j, Tb, L);
    }
  };
  int stamp = 0;
  if (T > 0)
    for (int d = 0; d < P.launches; ++d, ++stamp) {
      int k_lo, count;
      long_loss_forward_diagonal(P, d, &k_lo, &count);
      for (int k = k_lo; k < k_lo + count; ++k) {
        const int j = d - k;
        CHECK(j >= 0 && j < J, "forward tile (%d, %d)", k, j);
        seen[k * J + j] += 1;
        if (act(k, j)) alpha_reads(k, j, stamp, "alpha");
      }
      for (int k = k_lo; k < k_lo + count; ++k) {  // (writes after every read of the launch: tiles of one launch do not see each other)
        const int j = d - k;
        if (!act(k, j)) continue;
        if (k == 0) stat[j] = stamp;
        if (long_loss_has_right(L, k, UB)) col[k * J + j] = stamp;
        const size_t i = ck_at(k, j);
        CHECK(ck[i] < 0, "checkpoint (%d,%d) written twice", k, j);
        ck[i] = stamp; ck_who[i] = k * J + j;
      }
    }
  // the finish kernel: the checkpoint of the last tile in time of the last label block
  if (counted && Tb > 0) {
    const int k = L > 0 ? (L - 1) / UB : 0, j = (Tb - 1) / TF;
    const size_t i = ck_at(k, j);
    CHECK(act(k, j) && ck[i] >= 0 && ck_who[i] == k * J + j, "finish reads checkpoint (%d,%d), never written Tb=%d L=%d", k, j, Tb, L);
    CHECK(j + 1 >= J || !act(k, j + 1), "finish reads a checkpoint that is not the block's last Tb=%d L=%d", Tb, L);
  }
  ++stamp;
  if (T > 0)
    for (int e = 0; e < P.launches; ++e) {
      int d, k_lo, count;
      long_loss_backward_diagonal(P, e, &d, &k_lo, &count);
      // the recompute tiles
      for (int k = k_lo; k < k_lo + count; ++k) {
        const int j = d - k;
        seen[k * J + j] += 16;
        if (act(k, j)) alpha_reads(k, j, stamp, "recompute");
      }
      for (int k = k_lo; k < k_lo + count; ++k) {
        const int j = d - k;
        if (!act(k, j)) continue;
        for (int t = j * TF; t < (j + 1) * TF && t < Tb; ++t) {
          RingRow &r = ring[row_at(k, t)];
          CHECK(r.state == 0 || r.state == 3, "recompute (%d,%d) overwrites the row of t=%d (state %d) before its row stage Tb=%d L=%d K=%d J=%d TF=%d",
                k, j, r.t, r.state, Tb, L, K, J, TF);
          r.t = t; r.k = k; r.stamp = stamp; r.state = 1;
        }
      }
      ++stamp;
      // the beta tiles
      for (int k = k_lo; k < k_lo + count; ++k) {
        const int j = d - k;
        if (!act(k, j)) continue;
        for (int t = j * TF; t < (j + 1) * TF && t < Tb; ++t) {
          const RingRow &r = ring[row_at(k, t)];
          CHECK(r.t == t && r.k == k && r.state == 1 && r.stamp < stamp, "beta (%d,%d) reads a row that is not alpha of t=%d Tb=%d L=%d", k, j, t, Tb, L);
        }
        CHECK(stat[j] >= 0, "beta (%d,%d) reads statistics never written", k, j);
        if (k > 0) CHECK(col[(k - 1) * J + j] >= 0, "beta (%d,%d) reads an alpha column never written Tb=%d L=%d", k, j, Tb, L);
        if (long_loss_beta_has_right(Tb, L, k, j, TF, UB))
          CHECK(colb[k * J + j] >= 0 && colb[k * J + j] < stamp, "beta (%d,%d) reads a column not yet written Tb=%d L=%d", k, j, Tb, L);
        if (!long_loss_beta_fresh(Tb, j, TF))
          CHECK(rowb[k] >= 0 && rowb[k] < stamp, "beta (%d,%d) reads a row buffer not yet written Tb=%d L=%d", k, j, Tb, L);
        else
          CHECK(j + 1 >= J || !act(k, j + 1), "beta (%d,%d) starts afresh before a tile that ran Tb=%d L=%d", k, j, Tb, L);
      }
      for (int k = k_lo; k < k_lo + count; ++k) {
        const int j = d - k;
        if (!act(k, j)) continue;
        if (k > 0) colb[(k - 1) * J + j] = stamp;
        rowb[k] = stamp;
        for (int t = j * TF; t < (j + 1) * TF && t < Tb; ++t) ring[row_at(k, t)].state = 2;
      }
      ++stamp;
      // the row stage of time block d
      if (d < J) {
        const int j = d;
        for (int t = j * TF; t < (j + 1) * TF && t < T; ++t) {
          grad_rows[t] += 1;
          if (!counted || t >= Tb) continue;  // zeros
          CHECK(act(0, j) && stat[j] >= 0, "row stage reads statistics never written t=%d Tb=%d L=%d", t, Tb, L);
          for (int k = 0; k < K && (k == 0 || k * UB < L); ++k) {
            if (!act(k, j)) continue;
            RingRow &r = ring[row_at(k, t)];
            CHECK(r.t == t && r.k == k && r.state == 2 && r.stamp < stamp, "row stage reads a row that is not the posteriors of (%d, t=%d): t=%d state %d Tb=%d L=%d",
                  k, t, r.t, r.state, Tb, L);
            r.state = 3;
          }
        }
        ++stamp;
      }
    }
  if (T > 0)
    for (int q = 0; q < K * J; ++q) CHECK(seen[q] == 17, "tile %d on %d forward and %d backward launches", q, seen[q] & 15, seen[q] >> 4);
  for (int t = 0; t < T; ++t) CHECK(grad_rows[t] == 1, "gradient row t=%d written %d times T=%d TF=%d", t, grad_rows[t], T, TF);
  for (const RingRow &r : ring) CHECK(r.state == 0 || r.state == 3, "a saved row of (%d, t=%d) was never read by the row stage Tb=%d L=%d", r.k, r.t, Tb, L);
}

int main() {
  // 1. regions
  const int shapes[][3] = {{0, 0, 0}, {1, 0, 5}, {1, 7, 0}, {2, 5, 4}, {3, 1300, 1025}, {2, 2600, 2100}, {1, 30000, 8192}, {8, 30000, 8192},
                           {1, 180000, 50000}, {3, 30000, 65536}, {8, 180000, 65536}, {1, 100, 3000}, {2, 129, 2049}};
  for (const auto &s : shapes)
    for (int kind = 0; kind < 2; ++kind)
      for (int tf : {0, 4, 64, 128, 1000, 1300}) check_regions(kind, s[0], s[1], s[2], tf);
  LongLossPlan P, Q;
  CHECK(long_loss_ckpt_plan(0, 1, 30000, 8192, 0, 1, &P) && P.total == (size_t)170923264u, "B=1 T=30000 U=8192 classic: %zu bytes", P.total);
  CHECK(long_loss_ckpt_plan(0, 1, 180000, 50000, 0, 1, &P) && long_loss_plan(0, 1, 180000, 50000, 0, 1, &Q) && P.K == 49 && P.J == 1407 &&
        P.total == (size_t)6385200384ull && P.total * 20 < Q.total, "an hour of audio: %zu bytes against %zu", P.total, Q.total);
  print_terms("classic   ", 0, 1, 30000, 8192, 0);
  print_terms("simplified", 1, 1, 30000, 8192, 0);
  print_terms("classic   ", 0, 8, 30000, 8192, 0);
  print_terms("classic   ", 0, 1, 8192, 1024, 0);
  print_terms("classic   ", 0, 1, 180000, 50000, 0);
  print_terms("simplified", 1, 1, 180000, 50000, 0);
  print_terms("classic   ", 0, 1, 180000, 50000, 32);
  print_terms("classic   ", 0, 1, 180000, 50000, 512);
  // what the plan refuses: what long_loss_plan refuses
  CHECK(!long_loss_ckpt_plan(2, 1, 5, 4, 0, 1, &P) && !long_loss_ckpt_plan(0, 1, 5, 4, 3, 1, &P) && !long_loss_ckpt_plan(0, 1, 5, 65537, 0, 1, &P) &&
        !long_loss_ckpt_plan(0, -1, 5, 4, 0, 1, &P) && !long_loss_ckpt_plan(0, 1 << 30, 1024, 65536, 4, 0, &P), "refusals");
  CHECK(!long_loss_ckpt_plan(0, 1 << 20, 1 << 14, 4, 0, 1, &P) && long_loss_ckpt_plan(0, 1 << 20, 1 << 13, 4, 0, 0, &P), "the row stage's grid");

  // 2. and 3. small grids, all lengths: blocks of UB = 8 positions, tiles of 4, 8 and 12 frames, up to 4 x 17 tiles (J < K, J == K,
  // J > K: the ring wraps)
  long replays = 0;
  for (int UB : {8})
    for (int TF : {4, 8, 12})
      for (int U : {0, 1, 8, 9, 16, 17, 30})
        for (int T : {1, 4, 5, 12, 13, 24, 33, 67}) {
          for (int Tb = 0; Tb <= T; ++Tb)
            for (int L = 0; L <= U; ++L, ++replays) replay(U, T, TF, UB, Tb, L);
        }
  replay(5, 0, 4, 8, 0, 0);
  replay(5, 0, 4, 8, 0, 3);
  replays += 2;
  // the real block, lengths around every boundary
  for (int TF : {4, 64, 128, 1300})
    for (int Tb : {0, 1, 127, 128, 129, 1023, 1024, 1025, 1200, 2047, 2048, 2049, 2300, 2600})
      for (int L : {0, 1, 900, 1023, 1024, 1025, 1500, 2047, 2048, 2049, 2100}) {
        replay(2100, 2600, TF, LONG_UB, Tb, L);
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
