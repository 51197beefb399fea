// Pieces the Parquet page kernels share (parquet.hip, parquet_nested.hip): the
// error codes, unaligned little-endian loads and the block-cooperative decoder
// of RLE / bit-packed hybrid streams (levels, dictionary indices, booleans).
//
// RLE / bit-packed hybrid streams are decoded block-cooperatively: lane 0 of
// the workgroup parses up to kRunCap run headers into LDS, then all 256 lanes
// decode values by binary search over the run starts.
#pragma once

#include "common.h"

namespace igloo {
namespace kern {
namespace {

constexpr int kRunCap = 512;

enum : int {
  PQ_ERR_RLE = 1,
  PQ_ERR_DICT_INDEX = 2,
  PQ_ERR_BYTE_ARRAY = 3,
  PQ_ERR_SNAPPY = 4,
  PQ_ERR_SNAPPY_SIZE = 5,
  PQ_ERR_DECIMAL = 6,
  PQ_ERR_ENCODING = 7,
  PQ_ERR_NULLS = 8,
  PQ_ERR_TRUNCATED = 9,
  PQ_ERR_REP_ROWS = 10,     // repetition levels disagree with the row count
  PQ_ERR_LEVEL_RANGE = 11,  // level out of range
};

__device__ inline void set_error(int* err, int code) { atomicCAS(err, 0, code); }

__device__ inline uint32_t ld_u32(const uint8_t* p) {
  if ((((uintptr_t)p) & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ inline uint64_t ld_u64(const uint8_t* p) {
  if ((((uintptr_t)p) & 7) == 0) return *reinterpret_cast<const uint64_t*>(p);
  return (uint64_t)ld_u32(p) | ((uint64_t)ld_u32(p + 4) << 32);
}

struct RleTable {
  int32_t start[kRunCap + 1];
  uint32_t val[kRunCap];
  int64_t ptr[kRunCap];  // bit-packed run: data address; RLE run: 0
  int64_t cur;
  int32_t done;
  int32_t nruns;
  int32_t err;
};

// Decode `count` values of an RLE / bit-packed hybrid stream [p, end) with bit
// width bw (0..32). sink(i, v) runs once per value index i in [0, count), on
// some lane of the block. Must be called by every lane; ends synchronised.
template <typename Sink>
__device__ bool rle_decode(const uint8_t* p, const uint8_t* end, int bw, int count, RleTable& t, Sink sink) {
  const int nbytes = (bw + 7) >> 3;
  const uint32_t mask = bw >= 32 ? 0xffffffffu : ((1u << bw) - 1u);
  if (threadIdx.x == 0) {
    t.cur = (int64_t)p;
    t.done = 0;
    t.err = 0;
  }
  __syncthreads();
  for (;;) {
    if (threadIdx.x == 0) {
      const uint8_t* q = (const uint8_t*)t.cur;
      int done = t.done, nr = 0;
      while (nr < kRunCap && done < count) {
        uint32_t h = 0;
        int sh = 0;
        bool ok = false;
        while (q < end && sh <= 28) {
          const uint8_t b = *q++;
          h |= (uint32_t)(b & 0x7f) << sh;
          if (!(b & 0x80)) {
            ok = true;
            break;
          }
          sh += 7;
        }
        if (!ok) {
          t.err = 1;
          break;
        }
        const int64_t left = count - done;
        int64_t n;
        t.start[nr] = done;
        if (h & 1) {
          const int64_t groups = h >> 1;
          n = groups * 8;
          const int64_t bytes = groups * bw;
          const int64_t need = left < n ? left : n;
          if (bw > 0 && (int64_t)(end - q) * 8 < need * bw) {  // truncated run
            t.err = 1;
            break;
          }
          t.ptr[nr] = bw > 0 ? (int64_t)q : 0;
          t.val[nr] = 0;
          q += bytes < (int64_t)(end - q) ? bytes : (int64_t)(end - q);
        } else {
          n = h >> 1;
          if (n == 0 || q + nbytes > end) {
            t.err = 1;
            break;
          }
          uint32_t v = 0;
          for (int b = 0; b < nbytes; ++b) v |= (uint32_t)q[b] << (8 * b);
          q += nbytes;
          t.ptr[nr] = 0;
          t.val[nr] = v & mask;
        }
        done += (int)(left < n ? left : n);
        ++nr;
      }
      t.start[nr] = done;
      t.nruns = nr;
      t.cur = (int64_t)q;
      t.done = done;
    }
    __syncthreads();
    const int nr = t.nruns;
    const int lo = t.start[0], hi = t.start[nr];
    if (t.err) return false;
    for (int i = lo + (int)threadIdx.x; i < hi; i += blockDim.x) {
      int a = 0, b = nr - 1;
      while (a < b) {
        const int m = (a + b + 1) >> 1;
        if (t.start[m] <= i) a = m;
        else b = m - 1;
      }
      uint32_t v;
      if (t.ptr[a] == 0) {
        v = t.val[a];
      } else {
        const int64_t bit = (int64_t)(i - t.start[a]) * bw;
        const uint8_t* q = (const uint8_t*)t.ptr[a] + (bit >> 3);
        const int sh = (int)(bit & 7);
        const int nb = (sh + bw + 7) >> 3;
        uint64_t w = 0;
        for (int k = 0; k < nb; ++k) w |= (uint64_t)q[k] << (8 * k);
        v = (uint32_t)(w >> sh) & mask;
      }
      sink(i, v);
    }
    const bool fin = hi >= count || nr == 0;
    __syncthreads();
    if (fin) return true;
  }
}

}  // namespace
}  // namespace kern
}  // namespace igloo
