// Two-argument moment aggregation: the count and the five second-order sums of
// (x, y) pairs per group in one pass over the two columns, for the regr_*
// family (igloo_amd/ops/moments.py). Part of the aggregate library the
// reference reaches through SessionContext::sql (reference
// crates/engine/src/lib.rs:54-57).
//
// The sums are taken around a per-group shift (Kx, Ky) = the group's first
// valid pair, so nothing cancels when |mean| is large against the spread:
//   Sx = sum(x - Kx), Sy = sum(y - Ky), Sxx = sum((x - Kx)^2),
//   Syy = sum((y - Ky)^2), Sxy = sum((x - Kx)(y - Ky)).
// The shift is a sample of the group, hence (K - mean)^2 <= sum((x - mean)^2)
// and M2 = Sxx - Sx^2 / n loses at most a factor 1 + n in condition. The
// finaliser (mean = K + S / n, M2x, M2y, Cxy) runs on the host side of the op
// over one element per group.
//
// Two launches:
//   A: first[g] = the smallest row index among the group's valid pairs;
//   B: the six states, reading (Kx, Ky) through first[]. Four regimes, as in
//      agg.hip, chosen on the host:
//      * no group ids or one group: registers -> wave reduction -> workgroup
//        combine in LDS -> one set of global adds per workgroup;
//      * few groups (kMomentsLdsMaxGroups): shifts and states in LDS per
//        workgroup, one merge per group and workgroup;
//      * non-decreasing group ids: each lane folds the runs of its
//        kMomChunk consecutive rows in registers and adds once per run; a
//        tile of one run is reduced across the wave first;
//      * otherwise: global atomic adds per row.
// A row is skipped when its validity byte is 0 or its group id lies outside
// [0, ngroups). The accumulation order of the float64 sums is free: results
// may differ in the last bits from run to run.
#include <limits>

#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace igloo {
namespace kern {

namespace {

constexpr int kMomChunk = 8;                       // rows per lane in the sorted regime
constexpr int kMomTile = kWave * kMomChunk;        // rows per wave there
static_assert(kMomTile == kMomentsRowsPerBlock, "the sorted regime runs one wave per workgroup");
// LDS words per group: Kx, Ky, count and the five sums
constexpr int kMomLdsWords = 8;
static_assert(kMomentsLdsMaxGroups * kMomLdsWords * 8 == kMomentsLdsBytes, "LDS bound follows the budget");

struct Mom {
  unsigned long long c;
  double sx, sy, sxx, syy, sxy;
};

struct MomOut {
  unsigned long long* cnt;
  double* sums;      // five arrays, `stride` elements apart: Sx, Sy, Sxx, Syy, Sxy
  int64_t stride;
};

__device__ inline void mom_zero(Mom& m) {
  m.c = 0;
  m.sx = m.sy = m.sxx = m.syy = m.sxy = 0.0;
}

__device__ inline void mom_row(Mom& m, double dx, double dy) {
  m.c += 1;
  m.sx += dx;
  m.sy += dy;
  m.sxx += dx * dx;
  m.syy += dy * dy;
  m.sxy += dx * dy;
}

__device__ inline void mom_merge(Mom& a, const Mom& b) {
  a.c += b.c;
  a.sx += b.sx;
  a.sy += b.sy;
  a.sxx += b.sxx;
  a.syy += b.syy;
  a.sxy += b.sxy;
}

// every lane ends with the wave's total
__device__ inline void mom_wave_fold(Mom& m) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    Mom o;
    o.c = __shfl_xor(m.c, off, kWave);
    o.sx = __shfl_xor(m.sx, off, kWave);
    o.sy = __shfl_xor(m.sy, off, kWave);
    o.sxx = __shfl_xor(m.sxx, off, kWave);
    o.syy = __shfl_xor(m.syy, off, kWave);
    o.sxy = __shfl_xor(m.sxy, off, kWave);
    mom_merge(m, o);
  }
}

// a register or LDS state into group g's global state (g inside [0, ngroups):
// every caller has checked it); a state without a pair adds nothing
__device__ inline void mom_emit(const MomOut& o, int64_t g, const Mom& m) {
  if (m.c == 0) return;
  atomicAdd(o.cnt + g, m.c);
  atomicAdd(o.sums + g, m.sx);
  atomicAdd(o.sums + o.stride + g, m.sy);
  atomicAdd(o.sums + 2 * o.stride + g, m.sxx);
  atomicAdd(o.sums + 3 * o.stride + g, m.syy);
  atomicAdd(o.sums + 4 * o.stride + g, m.sxy);
}

template <typename R>
constexpr R no_row() { return std::numeric_limits<R>::max(); }

__device__ inline void row_min(int32_t* p, int64_t i) { atomicMin(p, (int)i); }
__device__ inline void row_min(int64_t* p, int64_t i) { atomicMin((long long*)p, (long long)i); }

// ------------------------------------------------------------------ phase A
// One group: a thread's rows ascend, so its first valid row is its smallest.
template <typename R, bool HasGid, bool HasValid>
__global__ __launch_bounds__(kBlock) void mom_first_single_kernel(const int32_t* __restrict__ gid,
                                                                 const uint8_t* __restrict__ valid, int64_t n,
                                                                 R* __restrict__ first) {
  long long best = INT64_MAX;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (HasGid && gid[i] != 0) continue;
    if (HasValid && !valid[i]) continue;
    best = i;
    break;
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const long long o = __shfl_xor(best, off, kWave);
    best = o < best ? o : best;
  }
  __shared__ long long part[kWavesPerBlock];
  if (lane_id() == 0) part[threadIdx.x / kWave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWavesPerBlock; ++w) best = part[w] < best ? part[w] : best;
    if (best != INT64_MAX) row_min(first, best);
  }
}

// Several groups: the state only ever decreases, so a row at or past the value
// read (however stale) cannot lower it and takes no atomic.
template <typename R, bool HasValid>
__global__ __launch_bounds__(kBlock) void mom_first_kernel(const int32_t* __restrict__ gid,
                                                          const uint8_t* __restrict__ valid, int64_t n, int ngroups,
                                                          R* first) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (HasValid && !valid[i]) continue;
    const int g = gid[i];
    if ((unsigned)g >= (unsigned)ngroups) continue;
    if ((int64_t)__hip_atomic_load(first + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i)
      row_min(first + g, i);
  }
}

// ------------------------------------------------------------------ phase B
template <typename R, bool HasGid, bool HasValid>
__global__ __launch_bounds__(kBlock) void mom_single_kernel(const int32_t* __restrict__ gid,
                                                           const double* __restrict__ x,
                                                           const double* __restrict__ y,
                                                           const uint8_t* __restrict__ valid, int64_t n,
                                                           const R* __restrict__ first, MomOut o) {
  const R f = first[0];
  if (f == no_row<R>()) return;      // no valid pair (uniform over the grid)
  const double kx = x[f], ky = y[f];
  Mom m;
  mom_zero(m);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (HasGid && gid[i] != 0) continue;
    if (HasValid && !valid[i]) continue;
    mom_row(m, x[i] - kx, y[i] - ky);
  }
  mom_wave_fold(m);
  __shared__ Mom part[kWavesPerBlock];
  if (lane_id() == 0) part[threadIdx.x / kWave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWavesPerBlock; ++w) mom_merge(m, part[w]);
    mom_emit(o, 0, m);
  }
}

// LDS layout: Kx[G], Ky[G], count[G], sums[5][G]
template <typename R, bool HasValid>
__global__ __launch_bounds__(kBlock) void mom_lds_kernel(const int32_t* __restrict__ gid,
                                                        const double* __restrict__ x, const double* __restrict__ y,
                                                        const uint8_t* __restrict__ valid, int64_t n, int ngroups,
                                                        const R* __restrict__ first, MomOut o) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long mom_lds[];
  const int G = ngroups;
  double* kx = (double*)mom_lds;
  double* ky = kx + G;
  unsigned long long* cnt = mom_lds + 2 * (size_t)G;
  double* s = (double*)(mom_lds + 3 * (size_t)G);
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    const R f = first[g];
    const bool any = f != no_row<R>();
    kx[g] = any ? x[f] : 0.0;
    ky[g] = any ? y[f] : 0.0;
    cnt[g] = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k * G + g] = 0.0;
  }
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (HasValid && !valid[i]) continue;
    const int g = gid[i];
    if ((unsigned)g >= (unsigned)G) continue;
    const double dx = x[i] - kx[g], dy = y[i] - ky[g];
    atomicAdd(&cnt[g], 1ULL);
    atomicAdd(&s[g], dx);
    atomicAdd(&s[G + g], dy);
    atomicAdd(&s[2 * G + g], dx * dx);
    atomicAdd(&s[3 * G + g], dy * dy);
    atomicAdd(&s[4 * G + g], dx * dy);
  }
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    Mom m;
    m.c = cnt[g];
    m.sx = s[g];
    m.sy = s[G + g];
    m.sxx = s[2 * G + g];
    m.syy = s[3 * G + g];
    m.sxy = s[4 * G + g];
    mom_emit(o, g, m);
  }
}

// A lane's kMomChunk consecutive rows in 16-byte loads where the chunk is whole
// and aligned (one load per row would refetch every line kMomChunk times).
__device__ inline void mom_load_ints(const int32_t* p, int64_t r0, int64_t n, int g[kMomChunk]) {
  if (r0 + kMomChunk <= n && ((uintptr_t)(p + r0) & 15) == 0) {
    const int4 a = *(const int4*)(p + r0), b = *(const int4*)(p + r0 + 4);
    g[0] = a.x; g[1] = a.y; g[2] = a.z; g[3] = a.w;
    g[4] = b.x; g[5] = b.y; g[6] = b.z; g[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < kMomChunk; ++j) g[j] = r0 + j < n ? p[r0 + j] : -1;
  }
}

__device__ inline void mom_load_f64(const double* p, int64_t r0, int64_t n, double v[kMomChunk]) {
  if (r0 + kMomChunk <= n && ((uintptr_t)(p + r0) & 15) == 0) {
#pragma unroll
    for (int j = 0; j < kMomChunk; j += 2) {
      const double2 a = *(const double2*)(p + r0 + j);
      v[j] = a.x;
      v[j + 1] = a.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kMomChunk; ++j) v[j] = r0 + j < n ? p[r0 + j] : 0.0;
  }
}

// bit j: row r0 + j is inside the input and valid
__device__ inline unsigned mom_load_valid(const uint8_t* p, int64_t r0, int64_t n) {
  unsigned ok = 0;
  if (!p) {
#pragma unroll
    for (int j = 0; j < kMomChunk; ++j) ok |= r0 + j < n ? (1u << j) : 0u;
  } else if (r0 + kMomChunk <= n && ((uintptr_t)(p + r0) & 7) == 0) {
    const unsigned long long w = *(const unsigned long long*)(p + r0);
#pragma unroll
    for (int j = 0; j < kMomChunk; ++j) ok |= ((w >> (8 * j)) & 0xff) ? (1u << j) : 0u;
  } else {
#pragma unroll
    for (int j = 0; j < kMomChunk; ++j) ok |= (r0 + j < n && p[r0 + j]) ? (1u << j) : 0u;
  }
  return ok;
}

// Non-decreasing group ids, one wave per workgroup and kMomTile rows per step.
// Correct for any order of ids (the runs are found by comparing neighbours);
// sorted ids make them long.
template <typename R>
__global__ __launch_bounds__(kWave) void mom_sorted_kernel(const int32_t* __restrict__ gid,
                                                          const double* __restrict__ x, const double* __restrict__ y,
                                                          const uint8_t* __restrict__ valid, int64_t n, int ngroups,
                                                          const R* __restrict__ first, MomOut o) {
  const int lane = threadIdx.x;
  for (int64_t base = blockIdx.x * (int64_t)kMomTile; base < n; base += (int64_t)gridDim.x * kMomTile) {
    const int64_t r0 = base + (int64_t)lane * kMomChunk;
    int g[kMomChunk];
    double vx[kMomChunk], vy[kMomChunk];
    mom_load_ints(gid, r0, n, g);
    mom_load_f64(x, r0, n, vx);
    mom_load_f64(y, r0, n, vy);
    const unsigned ok = mom_load_valid(valid, r0, n);
    const int live = n - r0 >= kMomChunk ? kMomChunk : (n > r0 ? (int)(n - r0) : 0);
    // a whole tile of one group: fold in registers, reduce across the wave, add once
    const int g0 = __shfl(g[0], 0, kWave);
    bool same = live == kMomChunk;
#pragma unroll
    for (int j = 0; j < kMomChunk; ++j) same &= g[j] == g0;
    if (__all(same)) {
      if ((unsigned)g0 >= (unsigned)ngroups) continue;
      const R f = first[g0];
      Mom m;
      mom_zero(m);
      if (f != no_row<R>()) {
        const double kx = x[f], ky = y[f];
#pragma unroll
        for (int j = 0; j < kMomChunk; ++j)
          if (ok & (1u << j)) mom_row(m, vx[j] - kx, vy[j] - ky);
      }
      mom_wave_fold(m);
      if (lane == 0) mom_emit(o, g0, m);
      continue;
    }
    // the lane's own runs: one set of adds where the id changes and at the chunk's end
    Mom m;
    mom_zero(m);
    int cur = -1;
    double kx = 0.0, ky = 0.0;
#pragma unroll
    for (int j = 0; j < kMomChunk; ++j) {
      if (j >= live) break;
      if (j == 0 || g[j] != cur) {
        if (j > 0 && (unsigned)cur < (unsigned)ngroups) mom_emit(o, cur, m);
        mom_zero(m);
        cur = g[j];
        if ((unsigned)cur < (unsigned)ngroups) {
          const R f = first[cur];
          const bool any = f != no_row<R>();
          kx = any ? x[f] : 0.0;
          ky = any ? y[f] : 0.0;
        }
      }
      if ((ok & (1u << j)) && (unsigned)cur < (unsigned)ngroups) mom_row(m, vx[j] - kx, vy[j] - ky);
    }
    if (live > 0 && (unsigned)cur < (unsigned)ngroups) mom_emit(o, cur, m);
  }
}

template <typename R, bool HasValid>
__global__ __launch_bounds__(kBlock) void mom_global_kernel(const int32_t* __restrict__ gid,
                                                           const double* __restrict__ x,
                                                           const double* __restrict__ y,
                                                           const uint8_t* __restrict__ valid, int64_t n, int ngroups,
                                                           const R* __restrict__ first, MomOut o) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (HasValid && !valid[i]) continue;
    const int g = gid[i];
    if ((unsigned)g >= (unsigned)ngroups) continue;
    const R f = first[g];     // a valid row of the group exists: this one
    Mom m;
    mom_zero(m);
    mom_row(m, x[i] - x[f], y[i] - y[f]);
    mom_emit(o, g, m);
  }
}

}  // namespace

void agg_moments2(const int32_t* gid, int64_t n, int ngroups, const double* x, const double* y, const uint8_t* valid,
                  int64_t* cnt, void* first, bool first64, double* sums, int64_t sum_stride, bool sorted_gids,
                  hipStream_t stream) {
  if (n <= 0) return;
  if (!first64 && n >= INT32_MAX) throw std::runtime_error("agg_moments2: 32-bit row numbers need n < 2^31 - 1");
  if (sum_stride < (ngroups > 1 ? ngroups : 1)) throw std::runtime_error("agg_moments2: sums stride below the group count");
  const MomOut o{(unsigned long long*)cnt, sums, sum_stride};
  const dim3 b(kBlock);
  const bool single = gid == nullptr || ngroups <= 1;
  dispatch(wide{first64}, gid != nullptr, valid != nullptr, [&](auto r, auto hg, auto hv) {
    using R = type_of<decltype(r)>;
    constexpr bool HG = decltype(hg)::value, HV = decltype(hv)::value;
    if (single) {
      // 1024 workgroups stream the input; one set of adds each
      const dim3 g(grid_for(n, kMomentsRowsPerBlock, 1024));
      launch("moments_first_single", mom_first_single_kernel<R, HG, HV>, g, b, 0, stream, gid, valid, n, as<R>(first));
      launch("moments_single", mom_single_kernel<R, HG, HV>, g, b, 0, stream, gid, x, y, valid, n,
             as<R>((const void*)first), o);
      return;
    }
    if constexpr (HG) {
      launch("moments_first", mom_first_kernel<R, HV>, dim3(grid_for(n, kMomentsRowsPerBlock, 32768)), b, 0, stream, gid,
             valid, n, ngroups, as<R>(first));
      const R* f = as<R>((const void*)first);
      if (ngroups <= kMomentsLdsMaxGroups) {
        // fewer workgroups when the per-workgroup fill and merge are large
        const int64_t maxg = ngroups <= 64 ? 8192 : 2048;
        launch("moments_lds", mom_lds_kernel<R, HV>, dim3(grid_for(n, kMomentsRowsPerBlock, maxg)), b,
               (size_t)ngroups * kMomLdsWords * 8, stream, gid, x, y, valid, n, ngroups, f, o);
      } else if (sorted_gids) {
        launch("moments_sorted", mom_sorted_kernel<R>, dim3(grid_for(n, kMomTile, 131072)), dim3(kWave), 0, stream, gid,
               x, y, valid, n, ngroups, f, o);
      } else {
        launch("moments_global", mom_global_kernel<R, HV>, dim3(grid_for(n, kMomentsRowsPerBlock, 32768)), b, 0, stream,
               gid, x, y, valid, n, ngroups, f, o);
      }
    }
  });
}

}  // namespace kern
}  // namespace igloo
