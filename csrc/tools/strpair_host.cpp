// Stand-alone sanitizer driver for the two-operand string routines (strpair.hip: str_pair_int,
// lev_lds / lev_long with lev_dp) and the substr_index case of strfunc.hip: every buffer is
// allocated at its exact size, so a read or write one byte outside a row, the result, the
// counter or the scratch slab is an AddressSanitizer report. Rows mix ASCII, multi-byte and
// truncated UTF-8, lengths around the LDS cap, a 70,000-character row, broadcast sides, and a
// scratch smaller than the rows need. Distances are compared with a full-matrix oracle.
// Built and run by tests/test_strpair_host.py (no GPU).
#include "common.h"
#include <vector>
#include <random>
#include <cstdio>
#include <algorithm>
#include "strpair.inc"
#include "strfunc.inc"
using namespace igloo::kern;
struct Col { int64_t* off; uint8_t* data; int64_t n; };
static Col make(const std::vector<std::string>& v) {
  Col c; c.n = (int64_t)v.size(); c.off = new int64_t[v.size() + 1]; int64_t t = 0; c.off[0] = 0;
  for (size_t i = 0; i < v.size(); ++i) { t += v[i].size(); c.off[i + 1] = t; }
  c.data = new uint8_t[t]; t = 0;                       // exact size: ASan sees one byte past
  for (auto& s : v) { memcpy(c.data + t, s.data(), s.size()); t += s.size(); }
  return c;
}
static void drop(Col& c) { delete[] c.off; delete[] c.data; }
static std::vector<uint32_t> cps(const std::string& s) {   // the kernels' own stepping, for the oracle
  std::vector<uint32_t> o; const uint8_t* p = (const uint8_t*)s.data(); int64_t n = s.size();
  for (int64_t i = 0; i < n;) { uint8_t c = p[i]; int l = c < 0x80 ? 1 : (c >> 5) == 6 ? 2 : (c >> 4) == 14 ? 3 : (c >> 3) == 30 ? 4 : 1;
    if (i + l > n) l = n - i; uint32_t k = 0; for (int q = 0; q < l; ++q) k |= (uint32_t)p[i + q] << (8 * q); o.push_back(k); i += l; }
  return o;
}
static int64_t lev(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b) {
  std::vector<int64_t> prev(b.size() + 1), cur(b.size() + 1);
  for (size_t j = 0; j <= b.size(); ++j) prev[j] = j;
  for (size_t i = 1; i <= a.size(); ++i) { cur[0] = i;
    for (size_t j = 1; j <= b.size(); ++j) cur[j] = std::min({prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1])});
    std::swap(prev, cur); }
  return prev[b.size()];
}
template <class F> static void run_block(int bd, F f) { gridDim.x = 1; blockDim.x = bd; blockIdx.x = 0; for (int t = 0; t < bd; ++t) { threadIdx.x = t; f(); } }
int main() {
  std::mt19937 g(3);
  const char* alpha[] = {"a", "b", "c", " ", ",", "\xc3\xa9", "\xe2\x82\xac", "\xf0\x9f\x98\x80", "\xc3", "\xe2\x82", "\x80"};
  auto rnd = [&](int maxlen) { std::string s; int n = g() % (maxlen + 1); for (int i = 0; i < n; ++i) s += alpha[g() % 11]; return s; };
  auto asc = [&](int n) { std::string s; for (int i = 0; i < n; ++i) s += (char)('a' + g() % 4); return s; };
  long checked = 0;
  for (int round = 0; round < 60; ++round) {
    int n = round == 0 ? 0 : 1 + g() % 300;
    bool ba = round % 5 == 1, bb = round % 5 == 2;
    std::vector<std::string> A, B;
    for (int i = 0; i < (ba ? 1 : n); ++i) A.push_back(g() % 7 == 0 ? asc(120 + g() % 20) : g() % 2 ? asc(g() % 40) : rnd(30));
    for (int i = 0; i < (bb ? 1 : n); ++i) B.push_back(g() % 9 == 0 ? asc(126 + g() % 140) : g() % 2 ? asc(g() % 40) : rnd(30));
    if (n && !ba && !bb) { A[0] = asc(300); B[0] = asc(260) + "\xc3\xa9"; if (n > 1) { A[1] = std::string(70000, 'x'); B[1] = "abc"; } }
    Col a = make(A), b = make(B);
    // str_pair_int, every function
    int32_t* out = new int32_t[n];
    run_block(256, [&] { str_pair_int_kernel<kSpStrpos>(a.off, a.data, ba, b.off, b.data, bb, n, out); });
    run_block(256, [&] { str_pair_int_kernel<kSpContains>(a.off, a.data, ba, b.off, b.data, bb, n, out); });
    run_block(256, [&] { str_pair_int_kernel<kSpStartsWith>(a.off, a.data, ba, b.off, b.data, bb, n, out); });
    run_block(256, [&] { str_pair_int_kernel<kSpEndsWith>(a.off, a.data, ba, b.off, b.data, bb, n, out); });
    run_block(256, [&] { str_pair_int_kernel<kSpFindInSet>(a.off, a.data, ba, b.off, b.data, bb, n, out); });
    // levenshtein: LDS kernel, then the long kernel over an exact-size scratch
    unsigned long long left[2] = {0, 0};
    run_block(128, [&] { lev_lds_kernel(a.off, a.data, ba, b.off, b.data, bb, n, out, left); });
    if (left[0]) {
      for (int64_t lanes : {(int64_t)64, (int64_t)3}) {
        int32_t* o2 = new int32_t[n]; memcpy(o2, out, n * 4);
        int64_t cells = left[1] + 1; int32_t* scratch = new int32_t[lanes * cells];
        gridDim.x = (lanes + 63) / 64; blockDim.x = 64;
        for (unsigned bx = 0; bx < gridDim.x; ++bx) for (int t = 0; t < 64; ++t) { blockIdx.x = bx; threadIdx.x = t;
          lev_long_kernel(a.off, a.data, ba, b.off, b.data, bb, n, o2, scratch, lanes, cells); }
        // a scratch too small for some rows (a replayed size): they stay -1, nothing is written outside
        int64_t small = cells / 2 + 1; int32_t* s2 = new int32_t[lanes * small]; int32_t* o3 = new int32_t[n]; memcpy(o3, out, n * 4);
        for (unsigned bx = 0; bx < gridDim.x; ++bx) for (int t = 0; t < 64; ++t) { blockIdx.x = bx; threadIdx.x = t;
          lev_long_kernel(a.off, a.data, ba, b.off, b.data, bb, n, o3, s2, lanes, small); }
        if (lanes == 64) memcpy(out, o2, n * 4);
        delete[] o2; delete[] o3; delete[] scratch; delete[] s2;
      }
    }
    for (int i = 0; i < n; ++i) {
      int64_t w = lev(cps(A[ba ? 0 : i]), cps(B[bb ? 0 : i]));
      if (out[i] != w) { printf("MISMATCH round %d row %d: %d want %ld\n", round, i, out[i], (long)w); return 1; }
      ++checked;
    }
    // substr_index through the two-pass kernels
    for (int64_t n1 : {1, 2, -1, -3, 0, 99, -99}) for (const char* d : {"a", "aa", " ", "\xc3\xa9", "", "ab"}) {
      StrFnArgs fa{kSfSubstrIndex, n1, (const uint8_t*)d, (int64_t)strlen(d), (const uint8_t*)"", 0};
      int64_t* len = new int64_t[a.n];
      run_block(256, [&] { strfn_len_kernel(fa, a.off, a.data, a.n, len); });
      int64_t* noff = new int64_t[a.n + 1]; noff[0] = 0; for (int64_t i = 0; i < a.n; ++i) noff[i + 1] = noff[i] + len[i];
      uint8_t* o = new uint8_t[noff[a.n]];
      run_block(256, [&] { strfn_copy_kernel(fa, a.off, a.data, a.n, noff, o, noff[a.n]); });
      delete[] len; delete[] noff; delete[] o;
    }
    delete[] out; drop(a); drop(b);
  }
  printf("ok: %ld distances equal the full-matrix oracle, no sanitizer report\n", checked);
  return 0;
}
