// Stand-alone check of the tiled alignment's host plan (csrc/ctc_align_long_plan.h): the diagonal enumeration, the workspace
// offsets and their size_t arithmetic, for K and J up to the limits.  No HIP, no GPU: build with the host compiler, with
// -fsanitize=address,undefined when a sanitizer run is wanted, and run it.  Prints "ok" and returns 0, or says what is wrong.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ctc_align_long_plan.h"

using namespace ctc;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

typedef unsigned __int128 u128;
static u128 r256(u128 x) { return (x + 255) / 256 * 256; }

static void check_schedule(int T, int U, int tf) {
  LongPlan P;
  CHECK(long_plan(1, T, U, tf, &P), "T=%d U=%d tf=%d", T, U, tf);
  const int TF = tf ? tf : LONG_TF_DEFAULT;
  CHECK(P.TF == TF && P.K == (U > 0 ? (U + 1023) / 1024 : 1) && P.J == (T > 0 ? (T + TF - 1) / TF : 1), "K=%d J=%d", P.K, P.J);
  CHECK(P.launches == P.K + P.J - 1, "launches=%d", P.launches);
  CHECK((long long)P.K * 1024 >= U && (long long)P.J * TF >= T, "the grid covers the lattice");
  std::vector<int> when((size_t)P.K * P.J, -1);  // the launch every tile ran on
  for (int d = 0; d < P.launches; ++d) {
    int k_lo, count;
    long_diagonal(P, d, &k_lo, &count);
    CHECK(count >= 1 && count <= (P.K < P.J ? P.K : P.J), "d=%d count=%d", d, count);
    for (int k = k_lo; k < k_lo + count; ++k) {
      const int j = d - k;
      CHECK(k >= 0 && k < P.K && j >= 0 && j < P.J, "d=%d k=%d j=%d", d, k, j);
      if (k < 0 || k >= P.K || j < 0 || j >= P.J) continue;
      CHECK(when[(size_t)k * P.J + j] == -1, "tile (%d, %d) twice", k, j);
      // both neighbours it reads ran on the launch before
      if (k > 0) CHECK(when[(size_t)(k - 1) * P.J + j] == d - 1, "left of (%d, %d)", k, j);
      if (j > 0) CHECK(when[(size_t)k * P.J + j - 1] == d - 1, "before (%d, %d)", k, j);
      when[(size_t)k * P.J + j] = d;
    }
  }
  for (size_t i = 0; i < when.size(); ++i) CHECK(when[i] >= 0, "tile %zu never ran", i);
}

static void check_offsets(int B, int T, int U, int tf) {
  LongPlan P;
  if (!long_plan(B, T, U, tf, &P)) {
    CHECK(false, "B=%d T=%d U=%d tf=%d refused", B, T, U, tf);
    return;
  }
  const u128 b = B, t = T, k = P.K, j = P.J;
  const u128 sizes[6] = {b * k * t * 512, b * (k - 1) * t * 16, b * k * LONG_ROW_DOUBLES * 8, b * j * 8, b * t * 4, b * 4};
  const size_t offs[7] = {P.off_bp, P.off_col, P.off_row, P.off_lse, P.off_idx, P.off_flag, P.total};
  u128 o = 0;
  for (int r = 0; r < 6; ++r) {
    CHECK((u128)offs[r] == o, "region %d of B=%d T=%d U=%d tf=%d starts at %zu", r, B, T, U, tf, offs[r]);
    CHECK(offs[r] % 256 == 0, "region %d alignment", r);
    o = r256(o + sizes[r]);
  }
  CHECK((u128)P.total == o, "total %zu", P.total);
  if (B > 0 && T > 0) {
    // the last element each kernel addresses, with the kernels' own index expressions in size_t
    const size_t bl = (size_t)B - 1, kl = (size_t)P.K - 1, tl = (size_t)T - 1;
    const size_t bp_last = ((bl * P.K + kl) * (size_t)T + tl) * 64 + 63;
    CHECK((u128)bp_last * 8 + 8 <= sizes[0], "back-pointer index");
    if (P.K > 1) {
      const size_t col_last = ((bl * (P.K - 1) + (kl - 1)) * (size_t)T + tl) * 2 + 1;
      CHECK((u128)col_last * 8 + 8 <= sizes[1], "column index");
    }
    const size_t row_last = (bl * P.K + kl) * LONG_ROW_DOUBLES + 2 * LONG_UB;
    CHECK((u128)row_last * 8 + 8 <= sizes[2], "row index");
    CHECK((u128)(bl * P.J + (P.J - 1)) * 8 + 8 <= sizes[3], "LSE index");
  }
}

int main() {
  const int tfs[] = {0, 4, 8, 64, 128, 132, 256, 4096};
  // every K, J from 1 past K on both sides, and the largest J a call can ask for (T = 180 000 at 4 frames per tile)
  for (int K = 1; K <= 64; ++K)
    for (int tf : tfs) {
      const int TF = tf ? tf : LONG_TF_DEFAULT;
      const int Js[] = {1, 2, K - 1, K, K + 1, 100};
      for (int J : Js) {
        if (J < 1) continue;
        check_schedule(J * TF, K * 1024, tf);
        check_schedule(J * TF - (TF - 1), K * 1024 - 1023, tf);
      }
    }
  check_schedule(180000, 65536, 4);
  check_schedule(180000, 50000, 0);
  check_schedule(0, 0, 0);
  check_schedule(0, 65536, 0);
  check_schedule(7, 0, 4);

  const int Bs[] = {0, 1, 8, 256}, Ts[] = {0, 1, 127, 128, 129, 30000, 180000}, Us[] = {0, 1, 1024, 1025, 8192, 50000, 65536};
  for (int B : Bs)
    for (int T : Ts)
      for (int U : Us)
        for (int tf : tfs) check_offsets(B, T, U, tf);
  check_offsets(4096, 180000, 65536, 4);  // 2.4e13 bytes: far beyond 32 bits, well inside 64

  LongPlan P;
  CHECK(!long_plan(1, 10, 10, 3, &P) && !long_plan(1, 10, 10, -4, &P) && !long_plan(1, 10, 65537, 0, &P), "bad arguments pass");
  CHECK(!long_plan(-1, 10, 10, 0, &P) && !long_plan(1, -1, 10, 0, &P) && !long_plan(1, 10, -1, 0, &P), "negative sizes pass");
  CHECK(!long_plan(1 << 30, 1024, 65536, 4, &P), "a grid beyond 2^31 - 1 workgroups passes");
  CHECK(long_plan(2097151, 1024, 1024, 0, &P), "a grid just inside the limit is refused");

  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
