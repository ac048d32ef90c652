// Stand-alone check of the host plan of the tiled alignment with wildcard labels (csrc/ctc_align_long_wild_plan.h): the regions of
// the plain tiled plan at their offsets, the three per-frame regions behind them, their size_t arithmetic and the last element each
// kernel addresses there.  No HIP, no GPU: build with the host compiler, with -fsanitize=address,undefined when a sanitizer run is
// wanted, and run it.  Prints "ok" and returns 0, or says what is wrong.  (The schedule is long_plan_check.cpp's ground.)
#include <stdio.h>
#include <stdlib.h>

#include "ctc_align_long_wild_plan.h"

using namespace ctc;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

typedef unsigned __int128 u128;
static u128 r256(u128 x) { return (x + 255) / 256 * 256; }

static void check_offsets(int B, int T, int U, int tf) {
  LongWildPlan W;
  LongPlan P;
  if (!long_wild_plan(B, T, U, tf, &W) || !long_plan(B, T, U, tf, &P)) {
    CHECK(false, "B=%d T=%d U=%d tf=%d refused", B, T, U, tf);
    return;
  }
  // the plain plan, unchanged, in front
  CHECK(W.base.K == P.K && W.base.J == P.J && W.base.TF == P.TF && W.base.launches == P.launches, "grid of B=%d T=%d U=%d tf=%d", B, T, U, tf);
  CHECK(W.base.off_bp == P.off_bp && W.base.off_col == P.off_col && W.base.off_row == P.off_row && W.base.off_lse == P.off_lse &&
        W.base.off_idx == P.off_idx && W.base.off_flag == P.off_flag && W.base.total == P.total, "base offsets");
  const u128 b = B, t = T;
  const u128 sizes[3] = {b * t * 8, b * t * 4, b * t * 8};
  const size_t offs[4] = {W.off_max, W.off_arg, W.off_lp, W.total};
  u128 o = P.total;
  for (int r = 0; r < 3; ++r) {
    CHECK((u128)offs[r] == o, "region %d of B=%d T=%d U=%d tf=%d starts at %zu", r, B, T, U, tf, offs[r]);
    CHECK(offs[r] % 256 == 0, "region %d alignment", r);
    o = r256(o + sizes[r]);
  }
  CHECK((u128)W.total == o, "total %zu", W.total);
  CHECK(W.total >= P.total, "the per-frame regions lie behind the plain plan");
  if (B > 0 && T > 0) {
    // the last element the kernels address, with their own index expression in size_t: (size_t)b * T + t
    const size_t last = ((size_t)B - 1) * (size_t)T + ((size_t)T - 1);
    CHECK((u128)last * 8 + 8 <= sizes[0] && (u128)last * 4 + 4 <= sizes[1] && (u128)last * 8 + 8 <= sizes[2], "per-frame index");
    CHECK((u128)W.off_lp + (u128)last * 8 + 8 <= (u128)W.total, "the last per-frame element lies inside the workspace");
  }
}

int main() {
  const int tfs[] = {0, 4, 8, 64, 128, 132, 256, 4096};
  const int Bs[] = {0, 1, 8, 256}, Ts[] = {0, 1, 31, 32, 33, 127, 128, 129, 30000, 180000}, Us[] = {0, 1, 1024, 1025, 8192, 50000, 65536};
  for (int B : Bs)
    for (int T : Ts)
      for (int U : Us)
        for (int tf : tfs) check_offsets(B, T, U, tf);
  check_offsets(4096, 180000, 65536, 4);  // 2.4e13 bytes: far beyond 32 bits, well inside 64

  LongWildPlan W;
  CHECK(long_wild_plan(1, 30000, 8192, 0, &W) && W.total == 127094272u, "the header's worked example: %zu", W.total);
  CHECK(!long_wild_plan(1, 10, 10, 3, &W) && !long_wild_plan(1, 10, 10, -4, &W) && !long_wild_plan(1, 10, 65537, 0, &W), "bad arguments pass");
  CHECK(!long_wild_plan(-1, 10, 10, 0, &W) && !long_wild_plan(1, -1, 10, 0, &W) && !long_wild_plan(1, 10, -1, 0, &W), "negative sizes pass");
  CHECK(!long_wild_plan(1 << 30, 1024, 65536, 4, &W), "a grid beyond 2^31 - 1 workgroups passes");
  CHECK(long_wild_plan(2097151, 1024, 1024, 0, &W), "a grid just inside the limit is refused");

  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
