// Stand-alone sanitizer driver for the framed order statistics: the routines of
// csrc/kernels/window_select.h (sel_place, sel_descend, sel_loop) compiled as plain C++ under
// ASan / UBSan through the host shim (strpair_host_shim.h as common.h). It walks them the way
// window_select.hip does, one "thread" after another: every tile of T ranks is merged level by
// level in two buffers of the tile's exact size (the LDS of select_tile_kernel), the higher levels
// in the tree itself (select_merge_kernel), and every query runs the descent and, for frames of at
// most 64 rows, the loop. perm, each tile buffer, the tree, the values and the validity bytes are
// heap blocks of their exact size, so a read or write one element outside is an AddressSanitizer
// report; signed overflow and bad shifts are UBSan reports.
//
// stdin, whitespace-separated integers, any number of cases:
//   T n q                      tile size (a power of two), rows, queries
//   v[0..n)  ok[0..n)          values and validity (0 / 1)
//   q times: lo hi k0 k1 two   a frame, two ranks, whether the second is asked for
// stdout, one line per query: "a b c d": the rows from the descent (a, b) and from the loop (c, d;
// "x x" where the frame is wider than 64 rows). -1 = no such rank. Built and run by
// tests/test_winselect_host.py (no GPU).
#include "common.h"
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <vector>
#include "window_select.h"
using namespace igloo::kern;

static bool next(long long* v) { return scanf("%lld", v) == 1; }

int main() {
  long cases = 0, queries = 0;
  std::string out;
  char line[128];
  long long T, n, q;
  while (next(&T)) {
    if (!next(&n) || !next(&q) || T < 1 || (T & (T - 1)) || n < 0 || q < 0) { fprintf(stderr, "bad case header\n"); return 2; }
    int64_t* vals = new int64_t[n];
    uint8_t* ok = new uint8_t[n];
    long long x;
    for (long long i = 0; i < n; ++i) { if (!next(&x)) return 2; vals[i] = (int64_t)x; }
    for (long long i = 0; i < n; ++i) { if (!next(&x)) return 2; ok[i] = (uint8_t)(x != 0); }
    // the argsort of the caller: valid rows by (value, position)
    std::vector<int32_t> order;
    for (long long i = 0; i < n; ++i) if (ok[i]) order.push_back((int32_t)i);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return vals[a] < vals[b]; });
    const int64_t m = (int64_t)order.size();
    int32_t* perm = new int32_t[m];
    std::copy(order.begin(), order.end(), perm);
    int L = 0;
    while (((int64_t)1 << L) < m) ++L;
    int tile_levels = 0;
    while (((long long)1 << tile_levels) < T) ++tile_levels;
    int32_t* tree = new int32_t[(size_t)L * m];
    // select_tile_kernel
    for (int64_t t0 = 0; t0 < m && L > 0; t0 += T) {
      const int64_t cnt = std::min<int64_t>(T, m - t0);
      int32_t* buf[2] = {new int32_t[cnt], new int32_t[cnt]};
      std::copy(perm + t0, perm + t0 + cnt, buf[0]);
      for (int l = 1; l <= std::min(L, tile_levels); ++l) {
        const int32_t* src = buf[(l - 1) & 1];
        int32_t* dst = buf[l & 1];
        std::fill(dst, dst + cnt, -7);
        for (int64_t i = 0; i < cnt; ++i) {
          const int64_t d = sel_place(src, cnt, i, l - 1);
          if (d < 0 || d >= cnt || dst[d] != -7) { fprintf(stderr, "tile placement %" PRId64 " at level %d\n", d, l); return 3; }
          dst[d] = src[i];
        }
        std::copy(dst, dst + cnt, tree + (int64_t)(l - 1) * m + t0);
      }
      delete[] buf[0];
      delete[] buf[1];
    }
    // select_merge_kernel
    for (int l = tile_levels + 1; l <= L; ++l) {
      const int32_t* src = sel_level(perm, tree, m, l - 1);      // (T = 1: level 1 is merged from perm itself)
      int32_t* dst = tree + (int64_t)(l - 1) * m;
      std::fill(dst, dst + m, -7);
      for (int64_t i = 0; i < m; ++i) {
        const int64_t d = sel_place(src, m, i, l - 1);
        if (d < 0 || d >= m || dst[d] != -7) { fprintf(stderr, "placement %" PRId64 " at level %d\n", d, l); return 3; }
        dst[d] = src[i];
      }
    }
    for (long long k = 0; k < q; ++k) {
      long long lo, hi, k0, k1, two;
      if (!next(&lo) || !next(&hi) || !next(&k0) || !next(&k1) || !next(&two)) return 2;
      int64_t a = -1, b = -1, c = -1, d = -1;
      if (m > 0) sel_descend(perm, tree, L, m, n, lo, hi, k0, k1, two != 0, &a, &b);
      const bool narrow = hi < lo || (unsigned long long)hi - (unsigned long long)lo < 64;
      if (narrow) sel_loop(vals, ok, n, lo, hi, k0, k1, two != 0, &c, &d);
      if (narrow)
        snprintf(line, sizeof line, "%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", a, b, c, d);
      else
        snprintf(line, sizeof line, "%" PRId64 " %" PRId64 " x x\n", a, b);
      out += line;
      ++queries;
    }
    delete[] tree;
    delete[] perm;
    delete[] ok;
    delete[] vals;
    ++cases;
  }
  fwrite(out.data(), 1, out.size(), stdout);
  fprintf(stderr, "winselect_host: %ld cases, %ld queries, no sanitizer report\n", cases, queries);
  return 0;
}
