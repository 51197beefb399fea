// Order statistics over window frames: median / percentile_cont /
// percentile_disc ... OVER (any frame). A framed order statistic is neither a
// difference of prefixes nor a two-block table lookup (window.hip), so it gets a
// selection structure of its own. igloo_amd/ops/window.py frame_kth resolves, per
// row, the rows holding ranks k0 (and k1) among the valid values of the row's
// frame [lo, hi]; exec/window.py gathers the values there and finalises.
//
//   * win_frame_kth (frames of at most LOOP_MAX_WIDTH rows, the split of
//     win_frame_minmax): one lane per row counts, for each valid row of the
//     frame, the frame's valid rows before it in (value, position) order. No
//     tree, no sort.
//   * win_select_build + win_select_query (wider frames): a merge-sort tree over
//     value ranks (window_select.h). The caller's argsort gives perm (positions by
//     ascending value, m valid ones first). Level l holds the positions in runs of
//     2^l ranks, each run sorted by position; one thread per element finds its
//     place by a binary search in the sibling run.
//       - select_tile_kernel builds levels 1..11 of a tile of kSelectTile = 2048
//         positions inside LDS and writes each of them out, one launch for all.
//         LDS: two int32 buffers of a tile = 16 KiB per 256-thread workgroup. A CU
//         has 160 KiB, which would hold 10 such workgroups; its 32 wave slots hold
//         8, so the wave slots, not the LDS, bound the occupancy (8 workgroups =
//         32 waves per CU). A 4096 tile (32 KiB) would leave 5 workgroups (20
//         waves) to save one global pass out of about 13 at 10 M rows.
//       - select_merge_kernel builds each higher level from the one below in
//         global memory, one launch per level.
//       - select_query_kernel descends from the root with one lane per row: at a
//         node it counts, with two binary searches, the positions of the left
//         child that lie in [lo, hi] and turns left or right. After L steps the
//         rank r is known and perm[r] is the row. About L^2 dependent 4-byte loads
//         per row and rank, no LDS, no scratch; both ranks share the descent while
//         they take the same turn. (Fractional cascading would bring it to O(L):
//         not built here.)
//     Memory: ceil(log2 m) * 4 bytes per valid row, freed after the call.
// Floats arrive as their order-preserving int64 images (window.hip f64_ord), so
// values compare as plain int64 and NaN is the greatest value.
// Parity: DataFusion accepts every aggregate as a window function; the reference
// reaches it through SessionContext::sql (reference crates/engine/src/lib.rs:54-57).
#include "common.h"
#include "kernels.h"
#include "launch.h"
#include "window_select.h"

namespace igloo {
namespace kern {

namespace {

constexpr int kTileItems = kSelectTile / kBlock;
static_assert(kSelectTile % kBlock == 0, "a tile is a whole number of items per thread");

// levels 1..min(L, kSelectTileLevels) of one tile of ranks, built in LDS
__global__ __launch_bounds__(kBlock) void select_tile_kernel(const int32_t* __restrict__ perm, int64_t m, int L,
                                                             int32_t* __restrict__ tree) {
  __shared__ int32_t buf[2][kSelectTile];
  const int64_t t0 = (int64_t)blockIdx.x * kSelectTile;
  if (t0 >= m) return;
  const int64_t cnt = m - t0 < kSelectTile ? m - t0 : kSelectTile;
  for (int j = 0; j < kTileItems; ++j) {
    const int i = threadIdx.x + j * kBlock;
    if (i < cnt) buf[0][i] = perm[t0 + i];
  }
  __syncthreads();
  const int top = L < kSelectTileLevels ? L : kSelectTileLevels;
  for (int l = 1; l <= top; ++l) {
    const int32_t* src = buf[(l - 1) & 1];
    int32_t* dst = buf[l & 1];
    for (int j = 0; j < kTileItems; ++j) {
      const int i = threadIdx.x + j * kBlock;
      if (i < cnt) {
        const int64_t d = sel_place(src, cnt, i, l - 1);
        if (d >= 0 && d < cnt) dst[d] = src[i];
      }
    }
    __syncthreads();
    int32_t* out = tree + (int64_t)(l - 1) * m + t0;
    for (int j = 0; j < kTileItems; ++j) {
      const int i = threadIdx.x + j * kBlock;
      if (i < cnt) out[i] = dst[i];
    }
    // (the next level writes the other buffer, which the copy above does not read)
  }
}

// level `shift + 1` from level `shift`, both in global memory
__global__ __launch_bounds__(kBlock) void select_merge_kernel(const int32_t* __restrict__ src, int64_t m, int shift,
                                                              int32_t* __restrict__ dst) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t d = sel_place(src, m, i, shift);
    if (d >= 0 && d < m) dst[d] = src[i];
  }
}

__global__ __launch_bounds__(kBlock) void select_query_kernel(const int32_t* __restrict__ perm,
                                                              const int32_t* __restrict__ tree, int L, int64_t m,
                                                              int64_t n, const int64_t* __restrict__ lo,
                                                              const int64_t* __restrict__ hi,
                                                              const int64_t* __restrict__ k0,
                                                              const int64_t* __restrict__ k1,
                                                              int64_t* __restrict__ pos0, int64_t* __restrict__ pos1) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n) return;
  int64_t a, b;
  sel_descend(perm, tree, L, m, n, lo[r], hi[r], k0[r], k1 != nullptr ? k1[r] : -1, k1 != nullptr, &a, &b);
  pos0[r] = a;
  if (pos1 != nullptr) pos1[r] = b;
}

__global__ __launch_bounds__(kBlock) void frame_kth_kernel(const int64_t* __restrict__ vals,
                                                           const uint8_t* __restrict__ valid, int64_t n,
                                                           const int64_t* __restrict__ lo,
                                                           const int64_t* __restrict__ hi,
                                                           const int64_t* __restrict__ k0,
                                                           const int64_t* __restrict__ k1, int64_t* __restrict__ pos0,
                                                           int64_t* __restrict__ pos1) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n) return;
  int64_t a, b;
  sel_loop(vals, valid, n, lo[r], hi[r], k0[r], k1 != nullptr ? k1[r] : -1, k1 != nullptr, &a, &b);
  pos0[r] = a;
  if (pos1 != nullptr) pos1[r] = b;
}

}  // namespace

int win_select_tile() { return kSelectTile; }

int win_select_levels(int64_t m) {
  int L = 0;
  while (((int64_t)1 << L) < m) ++L;
  return L;
}

void win_select_build(const int32_t* perm, int64_t m, int levels, int32_t* tree, hipStream_t s) {
  if (m <= 1) return;
  if (m >= ((int64_t)1 << 31)) throw std::runtime_error("win_select_build: 2^31 or more rows");
  if (levels != win_select_levels(m)) throw std::runtime_error("win_select_build: levels do not match m");
  launch("win.select_tile", select_tile_kernel, dim3(grid_for(m, kSelectTile, INT32_MAX)), dim3(kBlock), 0, s, perm, m,
         levels, tree);
  for (int l = kSelectTileLevels + 1; l <= levels; ++l)
    launch("win.select_merge", select_merge_kernel, dim3(grid_for(m, kBlock, 1 << 16)), dim3(kBlock), 0, s,
           tree + (int64_t)(l - 2) * m, m, l - 1, tree + (int64_t)(l - 1) * m);
}

void win_select_query(const int32_t* perm, const int32_t* tree, int levels, int64_t m, int64_t n, const int64_t* lo,
                      const int64_t* hi, const int64_t* k0, const int64_t* k1, int64_t* pos0, int64_t* pos1,
                      hipStream_t s) {
  if (n == 0) return;
  if (m <= 1 || levels != win_select_levels(m)) throw std::runtime_error("win_select_query: bad tree shape");
  launch("win.select_query", select_query_kernel, dim3(grid_for(n, kBlock, INT32_MAX)), dim3(kBlock), 0, s, perm, tree,
         levels, m, n, lo, hi, k0, k1, pos0, k1 != nullptr ? pos1 : nullptr);
}

void win_frame_kth(const int64_t* vals, const uint8_t* valid, int64_t n, const int64_t* lo, const int64_t* hi,
                   const int64_t* k0, const int64_t* k1, int64_t* pos0, int64_t* pos1, hipStream_t s) {
  if (n == 0) return;
  launch("win.frame_kth", frame_kth_kernel, dim3(grid_for(n, kBlock, INT32_MAX)), dim3(kBlock), 0, s, vals, valid, n, lo,
         hi, k0, k1, pos0, k1 != nullptr ? pos1 : nullptr);
}

}  // namespace kern
}  // namespace igloo
