// Stand-alone check of the tiled edit counts' host plan (csrc/ctc_edit_long_plan.h): the diagonal enumeration, the workspace offsets
// and their size_t arithmetic for K and J up to the limits, and a host walk of the tiles that reads and writes a poisoned workspace
// of exactly plan.total bytes at the indices the kernel uses (ctc_edit_long.hip) and must reproduce the plain table.  No HIP, no
// GPU: build with the host compiler, with -fsanitize=address,undefined when a sanitizer run is wanted, and run it.  Prints "ok" and
// returns 0, or says what is wrong.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctc_edit_long_plan.h"

using namespace ctc;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

typedef unsigned __int128 u128;
typedef long long word;
static const word DEL = 1LL << 42, SUB = DEL + (1LL << 21), INS = DEL + 1;
static u128 r256(u128 x) { return (x + 255) / 256 * 256; }

static void check_schedule(int R, int stride, int rows) {
  EditCountsPlan P;
  CHECK(edit_counts_plan(1, 1, R, stride, rows, &P), "R=%d stride=%d rows=%d", R, stride, rows);
  const int RT = rows ? rows : EDIT_LONG_RT_DEFAULT;
  CHECK(P.RT == RT && P.K == (R > 0 ? (R + 1023) / 1024 : 1) && P.J == (stride > 0 ? (stride + RT - 1) / RT : 1), "K=%d J=%d", P.K, P.J);
  CHECK(P.launches == P.K + P.J - 1, "launches=%d", P.launches);
  CHECK(64 * P.NL >= (R < 1024 ? R : 1024) && (P.NL == 1 || 32 * P.NL < R) && (P.NL == 16 || P.K == 1), "NL=%d", P.NL);
  std::vector<int> when((size_t)P.K * P.J, -1);  // the launch every tile ran on
  for (int d = 0; d < P.launches; ++d) {
    int k_lo, count;
    edit_counts_diagonal(P, d, &k_lo, &count);
    CHECK(count >= 1 && count <= (P.K < P.J ? P.K : P.J), "d=%d count=%d", d, count);
    for (int k = k_lo; k < k_lo + count; ++k) {
      const int j = d - k;
      CHECK(k >= 0 && k < P.K && j >= 0 && j < P.J, "d=%d k=%d j=%d", d, k, j);
      if (k < 0 || k >= P.K || j < 0 || j >= P.J) continue;
      CHECK(when[(size_t)k * P.J + j] == -1, "tile (%d, %d) twice", k, j);
      if (k > 0) CHECK(when[(size_t)(k - 1) * P.J + j] == d - 1, "left of (%d, %d)", k, j);
      if (j > 0) CHECK(when[(size_t)k * P.J + j - 1] == d - 1, "above (%d, %d)", k, j);
      when[(size_t)k * P.J + j] = d;
    }
  }
  for (int v : when) CHECK(v >= 0, "a tile never ran");
}

static void check_bytes(int B, int N, int R, int stride) {
  EditCountsPlan P;
  CHECK(edit_counts_plan(B, N, R, stride, 0, &P), "B=%d N=%d R=%d stride=%d", B, N, R, stride);
  const u128 pairs = (u128)B * N, K = R > 0 ? (R + 1023) / 1024 : 1;
  const u128 col = r256(8 * pairs * (K - 1) * stride), row = r256(8 * pairs * K * 1024);
  CHECK(P.off_col == 0 && (u128)P.off_row == col && (u128)P.total == col + row, "offsets B=%d N=%d R=%d stride=%d", B, N, R, stride);
  CHECK(P.off_row % 256 == 0 && P.total % 256 == 0, "alignment");
}

// The tiles of one pair in launch order on a workspace filled with 0xFF, tile boundaries read and written where the kernel reads
// and writes them; inside a tile the plain recurrence.  Returns the packed word of cell (h, r).
static word walk(const EditCountsPlan &P, int pairs, int idx, const std::vector<int> &hyp, const std::vector<int> &ref, std::vector<char> &ws) {
  const int h = (int)hyp.size(), r = (int)ref.size(), UB = 64 * P.NL;
  CHECK(ws.size() == P.total && idx < pairs, "workspace");
  word *const cols = reinterpret_cast<word *>(ws.data() + P.off_col), *const rows = reinterpret_cast<word *>(ws.data() + P.off_row);
  const size_t ncols = (P.off_row - P.off_col) / 8, nrows_words = (P.total - P.off_row) / 8;
  word result = -1;
  int writers = 0;
  if (h == 0 || r == 0) return (word)(h + r) * DEL + (r == 0 ? h : 0);
  for (int d = 0; d < P.launches; ++d) {
    int k_lo, count;
    edit_counts_diagonal(P, d, &k_lo, &count);
    for (int k = k_lo; k < k_lo + count; ++k) {
      const int jt = d - k, j00 = k * UB, i0 = jt * P.RT;
      if (j00 >= r || i0 >= h) continue;
      const int nr = std::min(P.RT, h - i0), kl = (r - 1) / UB, width = k == kl ? r - j00 : UB;
      const size_t colp = ((size_t)idx * (P.K - 1) + (k > 0 ? k - 1 : 0)) * P.hyp_stride;
      const size_t colq = ((size_t)idx * (P.K - 1) + std::min(k, std::max(P.K - 2, 0))) * P.hyp_stride + i0;
      const size_t rowp = ((size_t)idx * P.K + k) * EDIT_LONG_UB;
      std::vector<word> prev(width + 1), cur(width + 1);
      if (jt == 0) prev[0] = (word)j00 * DEL;
      else if (k == 0) prev[0] = (word)i0 * INS;
      else { CHECK(colp + i0 - 1 < ncols, "corner"); prev[0] = cols[colp + i0 - 1]; }
      for (int j = 1; j <= width; ++j) {
        if (jt == 0) prev[j] = (word)(j00 + j) * DEL;
        else { CHECK(rowp + j - 1 < nrows_words, "row read"); prev[j] = rows[rowp + j - 1]; }
      }
      for (int i = 1; i <= nr; ++i) {
        if (k == 0) cur[0] = (word)(i0 + i) * INS;
        else { CHECK(colp + i0 + i - 1 < ncols, "column read"); cur[0] = cols[colp + i0 + i - 1]; }
        for (int j = 1; j <= width; ++j)
          cur[j] = std::min(std::min(prev[j] + INS, cur[j - 1] + DEL), prev[j - 1] + (hyp[i0 + i - 1] != ref[j00 + j - 1] ? SUB : 0));
        if (k < kl) { CHECK(colq + i - 1 < ncols && i0 + i - 1 < P.hyp_stride, "column write"); cols[colq + i - 1] = cur[width]; }
        prev.swap(cur);
      }
      if (i0 + nr < h) {
        for (int j = 1; j <= width; ++j) { CHECK(rowp + j - 1 < nrows_words, "row write"); rows[rowp + j - 1] = prev[j]; }
      } else if (k == kl) {
        result = prev[width];
        ++writers;
      }
    }
  }
  CHECK(writers == 1, "writers=%d h=%d r=%d", writers, h, r);
  return result;
}

static word plain(const std::vector<int> &hyp, const std::vector<int> &ref) {
  const int h = (int)hyp.size(), r = (int)ref.size();
  std::vector<word> prev(r + 1), cur(r + 1);
  for (int j = 0; j <= r; ++j) prev[j] = (word)j * DEL;
  for (int i = 1; i <= h; ++i) {
    cur[0] = (word)i * INS;
    for (int j = 1; j <= r; ++j) cur[j] = std::min(std::min(prev[j] + INS, cur[j - 1] + DEL), prev[j - 1] + (hyp[i - 1] != ref[j - 1] ? SUB : 0));
    prev.swap(cur);
  }
  return prev[r];
}

static void check_walk(int h, int r, int R, int stride, int rows, unsigned seed) {
  EditCountsPlan P;
  const int pairs = 3;
  CHECK(edit_counts_plan(1, pairs, R, stride, rows, &P), "plan");
  std::vector<char> ws(P.total, (char)0xFF);
  std::vector<int> hyp(h), ref(r);
  srand(seed);
  for (int &t : hyp) t = rand() % 3;
  for (int &t : ref) t = rand() % 3;
  const word got = walk(P, pairs, 1, hyp, ref, ws), want = plain(hyp, ref);
  CHECK(got == want, "h=%d r=%d R=%d stride=%d rows=%d: %lld != %lld", h, r, R, stride, rows, got, want);
}

int main() {
  for (int R : {0, 1, 64, 65, 512, 513, 1023, 1024, 1025, 2048, 2049, 65535, 65536})
    for (int stride : {0, 1, 63, 64, 65, 511, 512, 513, 70000, 1 << 20})
      for (int rows : {0, 64, 128, 2048, 1 << 20, 1 << 30}) check_schedule(R, stride, rows);
  for (int B : {0, 1, 3, 256})
    for (int N : {1, 7, 4096})
      for (int R : {0, 1, 1024, 1025, 3000, 65536})
        for (int stride : {0, 1, 70, 65536, 1 << 20}) check_bytes(B, N, R, stride);
  check_bytes(1 << 10, 1 << 10, 65536, 1 << 20);  // 2^59 bytes
  EditCountsPlan P;
  CHECK(!edit_counts_plan(1, 1, 65537, 5, 0, &P) && !edit_counts_plan(1, 1, 4, (1 << 20) + 1, 0, &P) && !edit_counts_plan(1, 1, 4, 5, 63, &P) &&
        !edit_counts_plan(1, 1, 4, 5, -64, &P) && !edit_counts_plan(1, 0, 4, 5, 0, &P) && !edit_counts_plan(1 << 16, 1 << 15, 4, 5, 0, &P) &&
        !edit_counts_plan(-1, 1, 4, 5, 0, &P), "limits");
  CHECK(edit_counts_plan((1 << 16), (1 << 15) - 1, 4, 5, 0, &P), "2^31 - 2^16 pairs");
  CHECK(!edit_counts_plan(1 << 14, 1 << 14, 65536, 65536, 1024, &P), "2^32 workgroups");
  unsigned seed = 1;
  for (int r : {1, 2, 100, 1023, 1024, 1025, 2047, 2048, 2049, 3000})
    for (int h : {1, 63, 64, 65, 128, 131, r - 1, r, r + 1})
      for (int rows : {64, 128, 0}) {
        if (h < 1) continue;
        check_walk(h, r, r, h, rows, seed++);
        check_walk(h, r, r + 700, h + 100, rows, seed++);
      }
  if (fails) { printf("%d failures\n", fails); return 1; }
  printf("ok\n");
  return 0;
}
