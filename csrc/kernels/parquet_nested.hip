// Parent rows of LIST / MAP / STRUCT Parquet columns from their Dremel levels
// (gfx950).
//
// A leaf of a repeated column carries one (repetition, definition) pair per
// ENTRY: an element, a NULL element, or the one placeholder of an empty or
// NULL list. pq_decode_kernel (parquet.hip) decodes the leaf as a flat column
// with one row per entry, so the child column lives in entry space and a list
// row is the view (first entry, entry count) into it; placeholders become NULL
// child rows that no list references. Entry positions count through every page
// and chunk of the leaf (the host planner sums the page headers' num_values),
// so a row whose entries cross a page or workgroup boundary is no special
// case. With rep_def = the definition level at the repeated node:
//   entry e opens a row          iff rep[e] == 0
//   the row has elements         iff def[e] >= rep_def      (else length 0)
//   the row is non-NULL          iff def[e] >= rep_def - 1
//
// Kernels (one workgroup per data page, PqLevelPage says where its streams are):
//   pq_level_count_kernel   opening entries of the page -> counts[page]; an
//                           exclusive scan of the counts (scan.hip) gives every
//                           page its first output row without a readback.
//   pq_list_rows_kernel     levels -> one flag byte per entry (global scratch),
//                           then an in-order block scan over the entries: every
//                           opening entry writes (start, has elements) and the
//                           row's validity. Row counts that disagree with the
//                           row groups set an error; every store is bounded by
//                           the row count n and the entry count E.
//   pq_list_lens_kernel     one lane per row: length = next row's start - start.
//   pq_struct_valid_kernel  STRUCT (no repetition): valid[row] = def >= anc_def.
#include "common.h"
#include "kernels.h"
#include "parquet_rle.h"

namespace igloo {
namespace kern {

namespace {

struct LevelStreams {
  const uint8_t* rep;
  const uint8_t* rep_end;
  const uint8_t* def;
  const uint8_t* def_end;
  bool ok;
};

// The page's repetition (has_rep) and definition streams. v1: both sit at the
// head of the payload behind 4-byte length prefixes (inside the decompression
// buffer when the page was compressed); v2: planned byte ranges of the raw buffer.
__device__ inline LevelStreams level_streams(const PqLevelPage& pg, const uint8_t* raw, const uint8_t* dec,
                                             bool has_rep) {
  LevelStreams s{nullptr, nullptr, nullptr, nullptr, true};
  if (!(pg.flags & PQ_LEVEL_V1)) {
    s.rep = raw + pg.rep_off;
    s.rep_end = s.rep + pg.rep_len;
    s.def = raw + pg.def_off;
    s.def_end = s.def + pg.def_len;
    return s;
  }
  const uint8_t* p = ((pg.flags & PQ_LEVEL_IN_DEC) ? dec : raw) + pg.rep_off;
  const uint8_t* end = p + pg.rep_len;
  if (has_rep) {
    if (end - p < 4 || (int64_t)ld_u32(p) > end - p - 4) {
      s.ok = false;
      return s;
    }
    s.rep = p + 4;
    s.rep_end = s.rep + ld_u32(p);
    p = s.rep_end;
  }
  if (end - p < 4 || (int64_t)ld_u32(p) > end - p - 4) {
    s.ok = false;
    return s;
  }
  s.def = p + 4;
  s.def_end = s.def + ld_u32(p);
  return s;
}

__device__ inline int block_sum(int v, int* red) {
  v = (int)wave_reduce_sum((int64_t)v);
  if (lane_id() == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < kWavesPerBlock; ++w) t += red[w];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(kBlock) void pq_level_count_kernel(const PqLevelPage* __restrict__ pages,
                                                                const uint8_t* __restrict__ raw,
                                                                const uint8_t* __restrict__ dec,
                                                                int32_t* __restrict__ counts, int* __restrict__ error) {
  __shared__ RleTable rt;
  __shared__ int red[kWavesPerBlock];
  const PqLevelPage pg = pages[blockIdx.x];
  const LevelStreams lv = level_streams(pg, raw, dec, true);
  if (!lv.ok) {
    if (threadIdx.x == 0) {
      set_error(error, PQ_ERR_TRUNCATED);
      counts[blockIdx.x] = 0;
    }
    return;
  }
  const bool chunk_start = pg.flags & PQ_LEVEL_CHUNK_START;
  int local = 0, bad = 0;
  const bool ok = rle_decode(lv.rep, lv.rep_end, 1, pg.num_entries, rt, [&](int i, uint32_t v) {
    local += v == 0;
    bad |= (v > 1) | (chunk_start && i == 0 && v != 0) << 1;   // a chunk starts with a row
  });
  const int total = ok ? block_sum(local, red) : 0;
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    if (!ok) set_error(error, PQ_ERR_RLE);
    else if (bad & 1) set_error(error, PQ_ERR_LEVEL_RANGE);
    else if (bad & 2) set_error(error, PQ_ERR_REP_ROWS);
    counts[blockIdx.x] = total;
  }
}

enum : int { kOpens = 1, kHasSlots = 2, kRowValid = 4 };

__global__ __launch_bounds__(kBlock) void pq_list_rows_kernel(
    const PqLevelPage* __restrict__ pages, int64_t npages, const uint8_t* __restrict__ raw,
    const uint8_t* __restrict__ dec, int max_def, int rep_def, const int64_t* __restrict__ row_base,
    uint8_t* __restrict__ flags, int64_t* __restrict__ data, uint8_t* __restrict__ valid, int64_t n, int64_t E,
    int* __restrict__ error) {
  __shared__ RleTable rt;
  __shared__ int64_t scan_ws[kWavesPerBlock + 1];
  const PqLevelPage pg = pages[blockIdx.x];
  const int ne = pg.num_entries;
  const int64_t e0 = pg.entry_base;
  int64_t row = row_base[blockIdx.x];
  // the opening entries of every chunk are its row group's rows, and of all chunks the n rows
  const bool rows_ok = !((pg.flags & PQ_LEVEL_CHUNK_START) && row != pg.first_row) &&
                       !(blockIdx.x == 0 && row_base[npages] != n);
  if (!rows_ok || e0 < 0 || ne < 0 || e0 + ne > E) {
    if (threadIdx.x == 0) set_error(error, PQ_ERR_REP_ROWS);
    return;
  }
  const LevelStreams lv = level_streams(pg, raw, dec, true);
  if (!lv.ok) {
    if (threadIdx.x == 0) set_error(error, PQ_ERR_TRUNCATED);
    return;
  }
  uint8_t* f = flags + e0;   // [e0, e0 + ne) is this page's own slice: checked against E above
  bool ok = rle_decode(lv.rep, lv.rep_end, 1, ne, rt, [&](int i, uint32_t v) { f[i] = v == 0 ? kOpens : 0; });
  int bad = 0;
  const uint32_t md = (uint32_t)max_def, rd = (uint32_t)rep_def;
  ok = ok && rle_decode(lv.def, lv.def_end, 32 - __clz(max_def), ne, rt, [&](int i, uint32_t v) {
         bad |= v > md;
         f[i] |= (v >= rd ? kHasSlots : 0) | (v + 1 >= rd ? kRowValid : 0);
       });
  bad = __syncthreads_or(bad);
  if (!ok || bad) {
    if (threadIdx.x == 0) set_error(error, ok ? PQ_ERR_LEVEL_RANGE : PQ_ERR_RLE);
    return;
  }
  // entries in order: the row of an opening entry = page base + opening entries before it
  for (int base = 0; base < ne; base += kBlock) {
    const int i = base + (int)threadIdx.x;
    const int fl = i < ne ? f[i] : 0;
    int64_t tot;
    const int64_t r = row + block_exclusive_scan(fl & kOpens, scan_ws, &tot);
    if ((fl & kOpens) && r >= 0 && r < n) {
      data[2 * r] = e0 + i;
      data[2 * r + 1] = (fl & kHasSlots) ? 1 : 0;
      if (valid) valid[r] = (fl & kRowValid) ? 1 : 0;
    }
    row += tot;
  }
}

__global__ __launch_bounds__(kBlock) void pq_list_lens_kernel(int64_t* __restrict__ data, int64_t n, int64_t E) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n) return;
  // starts (data[2r]) are only read here, lengths (data[2r + 1]) only written by their own lane
  const int64_t start = data[2 * r];
  const int64_t next = r + 1 < n ? data[2 * (r + 1)] : E;
  const int64_t len = next - start;
  data[2 * r + 1] = (data[2 * r + 1] != 0 && len > 0 && start >= 0 && next <= E) ? len : 0;
}

__global__ __launch_bounds__(kBlock) void pq_struct_valid_kernel(const PqLevelPage* __restrict__ pages,
                                                                 const uint8_t* __restrict__ raw,
                                                                 const uint8_t* __restrict__ dec, int max_def,
                                                                 int anc_def, uint8_t* __restrict__ valid, int64_t n,
                                                                 int* __restrict__ error) {
  __shared__ RleTable rt;
  const PqLevelPage pg = pages[blockIdx.x];
  const int ne = pg.num_entries;
  const int64_t r0 = pg.entry_base;   // no repetition: an entry is a row
  if (r0 < 0 || ne < 0 || r0 + ne > n) {
    if (threadIdx.x == 0) set_error(error, PQ_ERR_REP_ROWS);
    return;
  }
  const LevelStreams lv = level_streams(pg, raw, dec, false);
  if (!lv.ok) {
    if (threadIdx.x == 0) set_error(error, PQ_ERR_TRUNCATED);
    return;
  }
  int bad = 0;
  const uint32_t md = (uint32_t)max_def, ad = (uint32_t)anc_def;
  uint8_t* out = valid + r0;
  const bool ok = rle_decode(lv.def, lv.def_end, 32 - __clz(max_def), ne, rt, [&](int i, uint32_t v) {
    bad |= v > md;
    out[i] = v >= ad;
  });
  bad = __syncthreads_or(bad);
  if ((!ok || bad) && threadIdx.x == 0) set_error(error, ok ? PQ_ERR_LEVEL_RANGE : PQ_ERR_RLE);
}

}  // namespace

void pq_level_count(const PqLevelPage* pages, int64_t npages, const uint8_t* raw, const uint8_t* dec,
                    int32_t* counts, int* error, hipStream_t stream) {
  if (npages <= 0) return;
  hipLaunchKernelGGL(pq_level_count_kernel, dim3((unsigned)npages), dim3(kBlock), 0, stream, pages, raw, dec, counts,
                     error);
  check_launch("pq_level_count", stream);
}

void pq_list_rows(const PqLevelPage* pages, int64_t npages, const uint8_t* raw, const uint8_t* dec, int max_def,
                  int rep_def, const int64_t* row_base, uint8_t* flags, int64_t* data, uint8_t* valid, int64_t n,
                  int64_t E, int* error, hipStream_t stream) {
  if (npages <= 0) return;
  hipLaunchKernelGGL(pq_list_rows_kernel, dim3((unsigned)npages), dim3(kBlock), 0, stream, pages, npages, raw, dec,
                     max_def, rep_def, row_base, flags, data, valid, n, E, error);
  check_launch("pq_list_rows", stream);
}

void pq_list_lens(int64_t* data, int64_t n, int64_t E, hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(pq_list_lens_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, data,
                     n, E);
  check_launch("pq_list_lens", stream);
}

void pq_struct_valid(const PqLevelPage* pages, int64_t npages, const uint8_t* raw, const uint8_t* dec, int max_def,
                     int anc_def, uint8_t* valid, int64_t n, int* error, hipStream_t stream) {
  if (npages <= 0) return;
  hipLaunchKernelGGL(pq_struct_valid_kernel, dim3((unsigned)npages), dim3(kBlock), 0, stream, pages, raw, dec,
                     max_def, anc_def, valid, n, error);
  check_launch("pq_struct_valid", stream);
}

}  // namespace kern
}  // namespace igloo
