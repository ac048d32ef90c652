// Stand-alone check of the host plan of the tiled CTC loss (csrc/ctc_loss_long_plan.h): host code only, its own main.
//   c++ -std=c++17 -I tf_seq2seq_losses_amd/csrc tests/tools/long_loss_plan_check.cpp -o long_loss_plan_check && ./long_loss_plan_check
// builds the same with -fsanitize=address,undefined.  It checks
//   1. the regions: monotone offsets, 256-byte aligned, no overlap, sizes as the header of include/ctc_amd.h states them, also
//      beyond 2^31 and 2^32 bytes; the forward-only plan has no per-frame rows;
//   2. the schedules: every tile is on exactly one forward and one backward launch;
//   3. the dependencies, for small grids and ALL lengths (T_b, L): replaying the launches with the predicates the kernels use,
//      everything an alpha tile, the finish kernel, a beta tile or the row stage reads was written on an EARLIER launch.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ctc_loss_long_plan.h"

using namespace ctc;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static size_t r256(size_t x) { return (x + 255) / 256 * 256; }

static void check_regions(int kind, int B, int T, int U, int tf, int want_grad) {
  LongLossPlan P;
  CHECK(long_loss_plan(kind, B, T, U, tf, want_grad, &P), "kind=%d B=%d T=%d U=%d tf=%d", kind, B, T, U, tf);
  const size_t b = (size_t)B, t = (size_t)T, k = (size_t)(U > 0 ? (U + 1023) / 1024 : 1), S = kind == 0 ? 2 : 1;
  const size_t sizes[8] = {16 * b * (k - 1) * t, 8 * b * k * 2056, 16 * b * t, 8 * b, 4 * b,
                           want_grad ? 8 * b * (k - 1) * t : 0, want_grad ? 8 * b * k * 2056 : 0,
                           want_grad ? 8 * b * k * t * (S * 1024 + 2) : 0};
  const size_t offs[8] = {P.off_col, P.off_row, P.off_stat, P.off_logp, P.off_flag, P.off_colb, P.off_rowb, P.off_rows};
  size_t o = 0;
  for (int i = 0; i < 8; ++i) {
    CHECK(offs[i] == o && offs[i] % 256 == 0, "region %d at %zu, expected %zu (B=%d T=%d U=%d)", i, offs[i], o, B, T, U);
    o = r256(o + sizes[i]);
  }
  CHECK(P.total == o, "total %zu, expected %zu", P.total, o);
  CHECK((size_t)P.K == k && P.J == (T > 0 ? (T + P.TF - 1) / P.TF : 1) && P.launches == P.K + P.J - 1, "grid");
  if (!want_grad) CHECK(P.off_colb == P.total && P.off_rows == P.total, "forward only: no per-frame rows");
}

// one replay: UB label positions per block, K x J tiles of TF frames, an utterance of Tb frames and L labels
static void replay(int K, int J, int TF, int UB, int Tb, int L) {
  LongLossPlan P;
  P.K = K; P.J = J; P.TF = TF; P.launches = K + J - 1;
  // launch stamp of the last write, -1: never written.  Per (block, tile): every frame of an active tile is written together
  std::vector<int> stat(J, -1), col(K * J, -1), rowa(K, -1), rows(K * J, -1), colb(K * J, -1), rowb(K, -1);
  std::vector<int> seen(K * J, 0);
  int stamp = 0;
  auto act = [&](int k, int j) { return long_loss_tile_active(Tb, L, k, j, TF, UB); };
  for (int d = 0; d < P.launches; ++d, ++stamp) {
    int k_lo, count;
    long_loss_forward_diagonal(P, d, &k_lo, &count);
    for (int k = k_lo; k < k_lo + count; ++k) {
      const int j = d - k;
      CHECK(j >= 0 && j < J, "forward tile (%d, %d)", k, j);
      seen[k * J + j] += 1;
      if (!act(k, j)) continue;
      if (k > 0) {
        CHECK(stat[j] >= 0 && stat[j] < stamp, "alpha (%d,%d) reads statistics not yet written Tb=%d L=%d", k, j, Tb, L);
        CHECK(col[(k - 1) * J + j] >= 0 && col[(k - 1) * J + j] < stamp, "alpha (%d,%d) reads a column not yet written Tb=%d L=%d", k, j, Tb, L);
      }
      if (!long_loss_alpha_fresh(k, j, TF, UB))
        CHECK(rowa[k] >= 0 && rowa[k] < stamp, "alpha (%d,%d) reads a row buffer not yet written Tb=%d L=%d", k, j, Tb, L);
      else
        CHECK(j == 0 || !act(k, j - 1), "alpha (%d,%d) starts afresh behind a tile that ran Tb=%d L=%d", k, j, Tb, L);
    }
    for (int k = k_lo; k < k_lo + count; ++k) {  // (writes after every read of the launch: tiles of one launch do not see each other)
      const int j = d - k;
      if (!act(k, j)) continue;
      if (k == 0) stat[j] = stamp;
      if (long_loss_has_right(L, k, UB)) col[k * J + j] = stamp;
      rowa[k] = stamp;
      rows[k * J + j] = stamp;
    }
  }
  // the finish kernel
  const bool counted = L <= Tb;
  if (counted && L > 0) CHECK(rowa[(L - 1) / UB] >= 0, "finish reads the row buffer of block %d, never written Tb=%d L=%d", (L - 1) / UB, Tb, L);
  if (counted && L == 0 && Tb > 0) CHECK(rowa[0] >= 0, "finish reads the start state, never written Tb=%d", Tb);
  ++stamp;
  for (int e = 0; e < P.launches; ++e, ++stamp) {
    int d, k_lo, count;
    long_loss_backward_diagonal(P, e, &d, &k_lo, &count);
    for (int k = k_lo; k < k_lo + count; ++k) {
      const int j = d - k;
      seen[k * J + j] += 16;
      if (!act(k, j)) continue;
      CHECK(rows[k * J + j] >= 0, "beta (%d,%d) reads saved rows never written Tb=%d L=%d", k, j, Tb, L);
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
    }
  }
  for (int q = 0; q < K * J; ++q) CHECK(seen[q] == 17, "tile %d on %d forward and %d backward launches", q, seen[q] & 15, seen[q] >> 4);
  // the row stage: frame t of a feasible utterance reads block 0 and every block with labels whose tile ran
  if (counted)
    for (int t = 0; t < Tb; ++t) {
      const int j = t / TF;
      CHECK(act(0, j) && stat[j] >= 0, "row stage reads statistics never written t=%d Tb=%d L=%d", t, Tb, L);
      for (int k = 0; k < K && (k == 0 || k * UB < L); ++k)
        if (act(k, j)) CHECK(rows[k * J + j] >= 0, "row stage reads rows never written");
    }
}

int main() {
  // 1. regions
  const int shapes[][3] = {{0, 0, 0}, {1, 0, 5}, {1, 7, 0}, {2, 5, 4}, {3, 1300, 1025}, {2, 2600, 2100}, {1, 30000, 8192}, {8, 30000, 8192},
                           {1, 180000, 50000}, {3, 30000, 65536}, {8, 180000, 65536}};
  for (const auto &s : shapes)
    for (int kind = 0; kind < 2; ++kind)
      for (int g = 0; g < 2; ++g)
        for (int tf : {0, 4, 64, 128, 1000}) check_regions(kind, s[0], s[1], s[2], tf, g);
  LongLossPlan P;
  CHECK(long_loss_plan(0, 1, 30000, 8192, 0, 1, &P) && P.total > ((size_t)1 << 31) && P.total == (size_t)3941783808u,
        "B=1 T=30000 U=8192 classic with a gradient: %zu bytes", P.total);
  printf("classic    B=1 T=30000 U=8192: %zu bytes with a gradient", P.total);
  CHECK(long_loss_plan(0, 1, 30000, 8192, 0, 0, &P), "forward only");
  printf(", %zu without\n", P.total);
  CHECK(long_loss_plan(1, 1, 30000, 8192, 0, 1, &P), "simplified");
  printf("simplified B=1 T=30000 U=8192: %zu bytes with a gradient\n", P.total);
  CHECK(long_loss_plan(0, 1, 180000, 50000, 0, 1, &P) && P.total > ((size_t)1 << 36), "an hour of audio: %zu bytes", P.total);
  printf("classic    B=1 T=180000 U=50000: %zu bytes with a gradient", P.total);
  CHECK(long_loss_plan(0, 1, 180000, 50000, 0, 0, &P) && P.total < ((size_t)1 << 28), "an hour of audio, forward only: %zu bytes", P.total);
  printf(", %zu without\n", P.total);
  // what the plan refuses
  CHECK(!long_loss_plan(2, 1, 5, 4, 0, 1, &P) && !long_loss_plan(0, 1, 5, 4, 3, 1, &P) && !long_loss_plan(0, 1, 5, 65537, 0, 1, &P) &&
        !long_loss_plan(0, -1, 5, 4, 0, 1, &P) && !long_loss_plan(0, 1 << 30, 1024, 65536, 4, 0, &P), "refusals");
  CHECK(!long_loss_plan(0, 1 << 20, 1 << 14, 4, 0, 1, &P) && long_loss_plan(0, 1 << 20, 1 << 13, 4, 0, 0, &P), "the row stage's grid");

  // 2. and 3. small grids, all lengths: blocks of UB = 8 positions, tiles of 4, 8 and 12 frames, up to 4 x 9 tiles
  long replays = 0;
  for (int UB : {8})
    for (int TF : {4, 8, 12})
      for (int U : {0, 1, 8, 9, 16, 17, 30})
        for (int T : {1, 4, 5, 12, 13, 24, 33}) {
          const int K = U > 0 ? (U + UB - 1) / UB : 1, J = (T + TF - 1) / TF;
          for (int Tb = 0; Tb <= T; ++Tb)
            for (int L = 0; L <= U; ++L, ++replays) replay(K, J, TF, UB, Tb, L);
        }
  // the real block, lengths around every boundary
  for (int TF : {4, 64, 128, 1300})
    for (int Tb : {0, 1, 127, 128, 129, 1023, 1024, 1025, 1200, 2047, 2048, 2049, 2300, 2600})
      for (int L : {0, 1, 900, 1023, 1024, 1025, 1500, 2047, 2048, 2049, 2100}) {
        replay(3, (2600 + TF - 1) / TF, TF, LONG_UB, Tb, L);
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
