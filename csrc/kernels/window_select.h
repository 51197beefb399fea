// Element routines of the framed order statistics (window_select.hip): the
// placement step that builds one level of the merge-sort tree, the descent that
// answers "which row holds rank k of frame [lo, hi]", and the loop that answers
// the same for a narrow frame. Plain integer code over raw pointers: it compiles
// into the gfx950 kernels and, through csrc/tools/strpair_host_shim.h, as host
// C++ (csrc/tools/winselect_host.cpp, run under ASan / UBSan).
//
// The tree. perm[0, m) holds the positions (rows in the window-sorted order) of
// the m valid rows by ascending (value, position): perm[r] is the row of value
// rank r. Level l (1 <= l <= L, L = ceil(log2 m)) holds the same m positions in
// runs of 2^l consecutive ranks, every run sorted by position; level 0 is perm
// itself. The last run of a level is partial when m is no power of two. The
// levels 1..L lie one after another, m int32 each.
//
// Every read of a level goes through sel_at, which clamps the index to [0, m):
// whatever lo / hi / k a caller hands in, no read leaves the level.
#pragma once
#include <cstdint>

namespace igloo {
namespace kern {

// positions sorted inside LDS by one workgroup (levels 1..kSelectTileLevels of a tile)
constexpr int kSelectTileLevels = 11;
constexpr int kSelectTile = 1 << kSelectTileLevels;

__device__ inline int32_t sel_at(const int32_t* a, int64_t m, int64_t i) {
  return a[i < 0 ? 0 : (i >= m ? m - 1 : i)];
}

// how many of the ascending a[base, base + len) are < x (a: m elements, m > 0)
__device__ inline int64_t sel_lower(const int32_t* a, int64_t m, int64_t base, int64_t len, int64_t x) {
  int64_t b = 0, e = len;
  while (b < e) {
    const int64_t mid = b + ((e - b) >> 1);
    if ((int64_t)sel_at(a, m, base + mid) < x) b = mid + 1; else e = mid;
  }
  return b;
}

// how many of the ascending a[base, base + len) lie in [lo, hi] (lo <= hi)
__device__ inline int64_t sel_count(const int32_t* a, int64_t m, int64_t base, int64_t len, int64_t lo, int64_t hi) {
  return sel_lower(a, m, base, len, hi + 1) - sel_lower(a, m, base, len, lo);
}

// One merge step. src[0, m) holds runs of 2^shift elements, each ascending (the
// last may be partial); element i of src goes to the returned index of the level
// above, whose runs of 2^(shift+1) are the merged pairs: its offset inside its
// own run plus the number of smaller elements in the sibling run. Positions are
// distinct, so there are no ties; with repeated values the index still lies
// inside the pair, hence inside [0, m).
__device__ inline int64_t sel_place(const int32_t* src, int64_t m, int64_t i, int shift) {
  const int64_t half = (int64_t)1 << shift;
  const int64_t run = i >> shift, p = i & (half - 1);
  const int64_t sib = (run ^ 1) << shift;
  int64_t len = m - sib;
  len = len < 0 ? 0 : (len > half ? half : len);
  const int64_t c = len ? sel_lower(src, m, sib, len, sel_at(src, m, i)) : 0;
  return ((run >> 1) << (shift + 1)) + p + c;
}

__device__ inline const int32_t* sel_level(const int32_t* perm, const int32_t* tree, int64_t m, int l) {
  return l == 0 ? perm : tree + (int64_t)(l - 1) * m;
}

// rank k (0 <= k < count of the node) below the node of level l that starts at
// rank `base`: the row holding it, or -1 where the tree contradicts itself
__device__ inline int64_t sel_descend_one(const int32_t* perm, const int32_t* tree, int64_t m, int l, int64_t base,
                                          int64_t lo, int64_t hi, int64_t k) {
  for (; l > 0; --l) {
    const int64_t half = (int64_t)1 << (l - 1);
    const int64_t len = m - base < half ? m - base : half;
    const int64_t c = sel_count(sel_level(perm, tree, m, l - 1), m, base, len, lo, hi);
    if (k >= c) {
      k -= c;
      base += half;
      if (base >= m) return -1;
    }
  }
  const int64_t p = sel_at(perm, m, base);
  return (k == 0 && p >= lo && p <= hi) ? p : -1;
}

// The rows holding ranks k0 and k1 (two: k1 is asked for) among the valid rows
// of frame [lo, hi], -1 where the frame is malformed (lo < 0, hi >= n, hi < lo)
// or the rank is outside [0, count). One descent serves both ranks while they
// take the same turn. About L^2 dependent 4-byte loads per rank.
__device__ inline void sel_descend(const int32_t* perm, const int32_t* tree, int L, int64_t m, int64_t n, int64_t lo,
                                   int64_t hi, int64_t k0, int64_t k1, bool two, int64_t* p0, int64_t* p1) {
  *p0 = -1;
  *p1 = -1;
  if (m <= 0 || lo < 0 || hi >= n || hi < lo) return;
  const bool want0 = k0 >= 0, want1 = two && k1 >= 0;
  if (!want0 && !want1) return;
  const int64_t root = sel_count(sel_level(perm, tree, m, L), m, 0, m, lo, hi);
  const bool ok0 = want0 && k0 < root, ok1 = want1 && k1 < root;
  if (!ok0 && !ok1) return;
  int l = L;
  int64_t base = 0;
  if (ok0 && ok1) {
    for (; l > 0; --l) {
      const int64_t half = (int64_t)1 << (l - 1);
      const int64_t len = m - base < half ? m - base : half;
      const int64_t c = sel_count(sel_level(perm, tree, m, l - 1), m, base, len, lo, hi);
      const bool r0 = k0 >= c, r1 = k1 >= c;
      if (r0 != r1) break;          // the ranks part here: each goes on alone
      if (r0) {
        k0 -= c;
        k1 -= c;
        base += half;
        if (base >= m) return;
      }
    }
    if (l == 0) {                   // k0 == k1: one leaf
      const int64_t p = sel_at(perm, m, base);
      if (k0 == 0 && p >= lo && p <= hi) *p0 = *p1 = p;
      return;
    }
  }
  if (ok0) *p0 = sel_descend_one(perm, tree, m, l, base, lo, hi, k0);
  if (ok1) *p1 = sel_descend_one(perm, tree, m, l, base, lo, hi, k1);
}

// The same answer for a narrow frame, by counting: for each valid j of the frame,
// the valid rows of the frame before it in (value, position) order; j holds the
// rank equal to that count. O(w^2) compares, no tree and no sort.
__device__ inline void sel_loop(const int64_t* vals, const uint8_t* valid, int64_t n, int64_t lo, int64_t hi,
                                int64_t k0, int64_t k1, bool two, int64_t* p0, int64_t* p1) {
  *p0 = -1;
  *p1 = -1;
  if (lo < 0 || hi >= n || hi < lo) return;
  if (k0 < 0 && !(two && k1 >= 0)) return;
  for (int64_t j = lo; j <= hi; ++j) {
    if (valid != nullptr && !valid[j]) continue;
    const int64_t x = vals[j];
    int64_t c = 0;
    for (int64_t i = lo; i <= hi; ++i) {
      if (valid != nullptr && !valid[i]) continue;
      const int64_t y = vals[i];
      c += (y < x) || (y == x && i < j);
    }
    if (c == k0) *p0 = j;
    if (two && c == k1) *p1 = j;
  }
}

}  // namespace kern
}  // namespace igloo
