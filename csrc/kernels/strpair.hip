// String functions of two string operands per row over plain (offsets +
// bytes) UTF-8 columns: strpos / contains / starts_with / ends_with /
// find_in_set (string, string -> int32) and levenshtein (edit distance over
// code points).
//
// Operands follow str_concat2 (strexpr.hip): each side is (offsets, bytes,
// broadcast); a one-row column with broadcast = true serves a constant. All
// kernels are one lane per row, grid-stride, and never index outside a row's
// [off[i], off[i+1]): a multi-byte sequence cut off by the row end is clamped
// to the bytes the row has.
//
// str_levenshtein keeps ONE rolling DP row over the row's shorter operand
// (swapped per row) in LDS, lane-interleaved: cell j of lane t sits at
// cells[j * blockDim.x + t], so a wave's 64 accesses to cell j are 128
// consecutive bytes: 32 dwords on 32 different banks, two neighbouring lanes
// per dword. No two lanes meet on a bank at different dwords; whether the
// 16-bit halves of one dword are served together by ds_read_u16 /
// ds_write_b16 on gfx950 is NOT measured (32-bit cells would be conflict-free
// by construction at twice the LDS, 5 waves per CU; BASELINE.md finds the
// kernel latency-bound, not LDS-bound, as it stands). Cells are 16 bits: a distance is
// bounded by the LONGER side, so only rows whose longer side has at most
// 65,535 characters (and whose shorter side has at most kLevFastMax) take
// this path. LDS budget: kLevBlock (128) lanes x (kLevFastMax + 1 = 128)
// cells x 2 B = 32 KiB per workgroup -> 5 workgroups = 10 waves per CU of the
// 160 KiB; kLevFastMax = 127 covers the comment / name columns this engine
// sees (TPC-H comments: at most 117 bytes).
// Every other row gets -1 and is counted in a two-word device counter (rows
// left, the largest shorter side among them), which the host reads back once
// to size a global scratch; str_levenshtein_long then fills the -1 rows with
// the same DP routine over 32-bit cells, a fixed number of worker lanes each
// owning an interleaved slab of that scratch.
// Parity: DataFusion's string function library (datafusion-functions 48,
// reference Cargo.lock:1062), reached through SessionContext::sql
// (reference crates/engine/src/lib.rs:54-57).
#include "common.h"
#include "kernels.h"

namespace igloo {
namespace kern {

namespace {

constexpr int kLevBlock = 128;

// bytes of the character that starts at s[i], clamped to the row's end
__device__ __forceinline__ int char_bytes(const uint8_t* s, int64_t i, int64_t n) {
  const uint8_t c = s[i];
  int l = c < 0x80 ? 1 : (c >> 5) == 6 ? 2 : (c >> 4) == 14 ? 3 : (c >> 3) == 30 ? 4 : 1;
  if (i + l > n) l = (int)(n - i);
  return l;
}

// the character's bytes as one word: equal words <=> equal characters
__device__ __forceinline__ uint32_t char_key(const uint8_t* s, int64_t i, int l) {
  uint32_t k = s[i];
  for (int q = 1; q < l; ++q) k |= (uint32_t)s[i + q] << (8 * q);
  return k;
}

__device__ __forceinline__ bool bytes_eq(const uint8_t* x, const uint8_t* y, int64_t m) {
  for (int64_t q = 0; q < m; ++q)
    if (x[q] != y[q]) return false;
  return true;
}

// one instantiation per function (see strfunc.hip strfn_int_kernel: a runtime
// switch over the bodies in one kernel was mis-compiled there)
template <int FN>
__global__ __launch_bounds__(kBlock) void str_pair_int_kernel(const int64_t* __restrict__ oa,
                                                              const uint8_t* __restrict__ ca, bool ba,
                                                              const int64_t* __restrict__ ob,
                                                              const uint8_t* __restrict__ cb, bool bb, int64_t n,
                                                              int32_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ia = ba ? 0 : i, ib = bb ? 0 : i;
    const uint8_t* a = ca + oa[ia];
    const int64_t na = oa[ia + 1] - oa[ia];
    const uint8_t* b = cb + ob[ib];
    const int64_t nb = ob[ib + 1] - ob[ib];
    int32_t v = 0;
    if constexpr (FN == kSpStrpos) {
      // 1-based character position of the first occurrence of b in a, 0 when absent
      int64_t c = 0;
      v = nb == 0 ? 1 : 0;
      for (int64_t j = 0; nb > 0 && j + nb <= na; ++j) {
        if ((a[j] & 0xC0) != 0x80) ++c;
        if (bytes_eq(a + j, b, nb)) {
          v = (int32_t)c;
          break;
        }
      }
    } else if constexpr (FN == kSpContains) {
      v = nb == 0 ? 1 : 0;
      for (int64_t j = 0; nb > 0 && j + nb <= na; ++j) {
        if (bytes_eq(a + j, b, nb)) {
          v = 1;
          break;
        }
      }
    } else if constexpr (FN == kSpStartsWith) {
      v = nb <= na && bytes_eq(a, b, nb);
    } else if constexpr (FN == kSpEndsWith) {
      v = nb <= na && bytes_eq(a + (na - nb), b, nb);
    } else {
      // find_in_set(a, list b): 1-based index of the comma-separated entry of
      // b equal to a, compared in place; an entry never holds a comma
      int64_t st = 0;
      int32_t idx = 1;
      for (int64_t j = 0; j <= nb; ++j) {
        if (j == nb || b[j] == ',') {
          if (j - st == na && bytes_eq(b + st, a, na)) {
            v = idx;
            break;
          }
          st = j + 1;
          ++idx;
        }
      }
    }
    out[i] = v;
  }
}

// characters of s[0..n), stepping exactly as the DP below does; *ascii is
// cleared when a byte is not ASCII
__device__ int64_t lev_chars(const uint8_t* s, int64_t n, bool* ascii) {
  int64_t c = 0;
  for (int64_t i = 0; i < n; ++c) {
    if (s[i] >= 0x80) *ascii = false;
    i += char_bytes(s, i, n);
  }
  return c;
}

// where the DP row lives: LDS (16-bit cells) or a global scratch slab (32-bit
// cells), both interleaved by lane
struct LdsRow {
  uint16_t* base;
  int stride;
  __device__ __forceinline__ int32_t get(int64_t j) const { return base[j * stride]; }
  __device__ __forceinline__ void set(int64_t j, int32_t v) const { base[j * stride] = (uint16_t)v; }
};
struct GlobalRow {
  int32_t* base;
  int64_t stride;
  __device__ __forceinline__ int32_t get(int64_t j) const { return base[j * stride]; }
  __device__ __forceinline__ void set(int64_t j, int32_t v) const { base[j * stride] = v; }
};

// edit distance of s (the shorter side: sc >= 1 characters, sc + 1 cells of
// `row`) and t. ASCII: both sides are pure ASCII, bytes are characters.
template <bool ASCII, class Row>
__device__ int32_t lev_dp(const uint8_t* s, int64_t sn, int64_t sc, const uint8_t* t, int64_t tn, Row row) {
  for (int64_t j = 0; j <= sc; ++j) row.set(j, (int32_t)j);
  int32_t i = 0, left = (int32_t)sc;
  for (int64_t p = 0; p < tn;) {
    uint32_t kt;
    if constexpr (ASCII) {
      kt = t[p++];
    } else {
      const int l = char_bytes(t, p, tn);
      kt = char_key(t, p, l);
      p += l;
    }
    int32_t diag = i;      // cell 0 of the previous row
    ++i;
    row.set(0, i);
    left = i;
    int64_t j = 0;
    // j < sc: the row has sc + 1 cells whatever the bytes say
    for (int64_t q = 0; q < sn && j < sc;) {
      uint32_t ks;
      if constexpr (ASCII) {
        ks = s[q++];
      } else {
        const int l = char_bytes(s, q, sn);
        ks = char_key(s, q, l);
        q += l;
      }
      ++j;
      const int32_t up = row.get(j);
      const int32_t sub = diag + (ks != kt);
      int32_t v = (up < left ? up : left) + 1;
      if (sub < v) v = sub;
      row.set(j, v);
      diag = up;
      left = v;
    }
  }
  return left;
}

struct LevRow {
  const uint8_t *s, *t;     // shorter / longer side
  int64_t sn, tn, sc, tc;   // bytes and characters of each
  bool ascii;
};

__device__ __forceinline__ LevRow lev_row(const int64_t* oa, const uint8_t* ca, bool ba, const int64_t* ob,
                                          const uint8_t* cb, bool bb, int64_t i) {
  const int64_t ia = ba ? 0 : i, ib = bb ? 0 : i;
  LevRow r;
  r.s = ca + oa[ia];
  r.sn = oa[ia + 1] - oa[ia];
  r.t = cb + ob[ib];
  r.tn = ob[ib + 1] - ob[ib];
  r.ascii = true;
  r.sc = lev_chars(r.s, r.sn, &r.ascii);
  r.tc = lev_chars(r.t, r.tn, &r.ascii);
  if (r.sc > r.tc) {
    const uint8_t* p = r.s;
    r.s = r.t;
    r.t = p;
    int64_t x = r.sn;
    r.sn = r.tn;
    r.tn = x;
    x = r.sc;
    r.sc = r.tc;
    r.tc = x;
  }
  return r;
}

__global__ __launch_bounds__(kLevBlock) void lev_lds_kernel(const int64_t* __restrict__ oa,
                                                            const uint8_t* __restrict__ ca, bool ba,
                                                            const int64_t* __restrict__ ob,
                                                            const uint8_t* __restrict__ cb, bool bb, int64_t n,
                                                            int32_t* __restrict__ out,
                                                            unsigned long long* __restrict__ left) {
  __shared__ uint16_t cells[(kLevFastMax + 1) * kLevBlock];
  const LdsRow row{cells + threadIdx.x, kLevBlock};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const LevRow r = lev_row(oa, ca, ba, ob, cb, bb, i);
    if (r.sc == 0) {
      out[i] = (int32_t)r.tc;
    } else if (r.sc > kLevFastMax || r.tc > 65535) {
      out[i] = -1;
      atomicAdd(left, 1ULL);
      atomicMax(left + 1, (unsigned long long)r.sc);
    } else {
      out[i] = r.ascii ? lev_dp<true>(r.s, r.sn, r.sc, r.t, r.tn, row) : lev_dp<false>(r.s, r.sn, r.sc, r.t, r.tn, row);
    }
  }
}

// the rows lev_lds_kernel left at -1: lane w of `lanes` owns the cells
// scratch[j * lanes + w], j < cells. A row that needs more cells than the
// scratch has (sized from a replayed readback that does not match the data)
// stays -1.
__global__ __launch_bounds__(kWave) void lev_long_kernel(const int64_t* __restrict__ oa,
                                                         const uint8_t* __restrict__ ca, bool ba,
                                                         const int64_t* __restrict__ ob,
                                                         const uint8_t* __restrict__ cb, bool bb, int64_t n,
                                                         int32_t* __restrict__ out, int32_t* __restrict__ scratch,
                                                         int64_t lanes, int64_t cells) {
  const int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (w >= lanes) return;
  const GlobalRow row{scratch + w, lanes};
  for (int64_t i = w; i < n; i += lanes) {
    if (out[i] != -1) continue;
    const LevRow r = lev_row(oa, ca, ba, ob, cb, bb, i);
    if (r.sc == 0 || r.sc + 1 > cells) continue;
    out[i] = r.ascii ? lev_dp<true>(r.s, r.sn, r.sc, r.t, r.tn, row) : lev_dp<false>(r.s, r.sn, r.sc, r.t, r.tn, row);
  }
}

}  // namespace

void str_pair_int(int fn, const int64_t* oa, const uint8_t* ca, bool ba, const int64_t* ob, const uint8_t* cb, bool bb,
                  int64_t n, int32_t* out, hipStream_t s) {
  if (n == 0) return;
  dim3 g(grid_for(n, kBlock, 1 << 16)), b(kBlock);
  if (fn == kSpStrpos)
    hipLaunchKernelGGL(str_pair_int_kernel<kSpStrpos>, g, b, 0, s, oa, ca, ba, ob, cb, bb, n, out);
  else if (fn == kSpContains)
    hipLaunchKernelGGL(str_pair_int_kernel<kSpContains>, g, b, 0, s, oa, ca, ba, ob, cb, bb, n, out);
  else if (fn == kSpStartsWith)
    hipLaunchKernelGGL(str_pair_int_kernel<kSpStartsWith>, g, b, 0, s, oa, ca, ba, ob, cb, bb, n, out);
  else if (fn == kSpEndsWith)
    hipLaunchKernelGGL(str_pair_int_kernel<kSpEndsWith>, g, b, 0, s, oa, ca, ba, ob, cb, bb, n, out);
  else if (fn == kSpFindInSet)
    hipLaunchKernelGGL(str_pair_int_kernel<kSpFindInSet>, g, b, 0, s, oa, ca, ba, ob, cb, bb, n, out);
  else
    throw std::runtime_error("str_pair_int: bad function");
  check_launch("strpair.int", s);
}

void str_levenshtein(const int64_t* oa, const uint8_t* ca, bool ba, const int64_t* ob, const uint8_t* cb, bool bb,
                     int64_t n, int32_t* out, int64_t* left, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(lev_lds_kernel, dim3(grid_for(n, kLevBlock, 1 << 16)), dim3(kLevBlock), 0, s, oa, ca, ba, ob, cb,
                     bb, n, out, reinterpret_cast<unsigned long long*>(left));
  check_launch("strpair.lev", s);
}

void str_levenshtein_long(const int64_t* oa, const uint8_t* ca, bool ba, const int64_t* ob, const uint8_t* cb, bool bb,
                          int64_t n, int32_t* out, int32_t* scratch, int64_t lanes, int64_t cells, hipStream_t s) {
  if (n == 0 || lanes <= 0 || cells <= 0) return;
  hipLaunchKernelGGL(lev_long_kernel, dim3(grid_for(lanes, kWave)), dim3(kWave), 0, s, oa, ca, ba, ob, cb, bb, n, out,
                     scratch, lanes, cells);
  check_launch("strpair.lev_long", s);
}

}  // namespace kern
}  // namespace igloo
