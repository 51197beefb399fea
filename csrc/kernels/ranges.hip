// Sorted-key join primitives for clustered inputs (lineitem by l_orderkey,
// orders by o_orderkey, and every join output that preserved that order).
//
//   sorted_ranges: for each probe key, the range [lo, lo+cnt) of equal keys in
//     a non-decreasing build column — one lower-bound binary search, then a
//     short forward scan (TPC-H keys repeat <= 7 times) that falls back to a
//     second binary search for long runs. Replaces two torch.searchsorted
//     passes.
//   expand_ranges: the (probe row, build row) pairs of those ranges, output
//     parallel and load balanced: a workgroup owns 2048 consecutive outputs,
//     finds the probe rows overlapping them with two binary searches over the
//     exclusive offsets, stages those offsets in LDS and lets every lane
//     binary-search its outputs there; stores are coalesced. Replaces
//     torch.repeat_interleave + cumsum + index_select (one thread per probe
//     row writing its run: 17 ms for one 60M-pair expansion at SF100).
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace igloo {
namespace kern {

namespace {

constexpr int kExpItems = 8;
constexpr int kExpTile = kBlock * kExpItems;
constexpr int kScanRun = 16;

template <typename K>
__global__ __launch_bounds__(kBlock) void sorted_ranges_kernel(const K* __restrict__ big, int64_t nb,
                                                              const K* __restrict__ q,
                                                              const uint8_t* __restrict__ qvalid, int64_t nq,
                                                              int64_t* __restrict__ lo_out,
                                                              int64_t* __restrict__ cnt_out,
                                                              const K* __restrict__ fence, int64_t nf) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
    if (qvalid && !qvalid[i]) {
      lo_out[i] = 0;
      cnt_out[i] = 0;
      continue;
    }
    const K key = q[i];
    int64_t a = 0, b = nb;
    if (fence) {
      // fence[j] = big[j * kFence] (a 1/kFence sample small enough to stay in
      // L2 / MALL): its lower bound j brackets the answer to one kFence-row
      // window, so the search touches ~3 HBM lines instead of ~20
      int64_t fa = 0, fb = nf;
      while (fa < fb) {
        const int64_t m = (fa + fb) >> 1;
        if (fence[m] < key) fa = m + 1;
        else fb = m;
      }
      a = fa > 0 ? (fa - 1) * kFence : 0;
      b = fa * kFence < nb ? fa * kFence : nb;
    }
    while (a < b) {
      const int64_t m = (a + b) >> 1;
      if (big[m] < key) a = m + 1;
      else b = m;
    }
    int64_t e = a;
    int k = 0;
    while (e < nb && k < kScanRun && big[e] == key) {
      ++e;
      ++k;
    }
    if (k == kScanRun && e < nb && big[e] == key) {
      int64_t a2 = e, b2 = nb;
      while (a2 < b2) {
        const int64_t m = (a2 + b2) >> 1;
        if (big[m] <= key) a2 = m + 1;
        else b2 = m;
      }
      e = a2;
    }
    lo_out[i] = a;
    cnt_out[i] = e - a;
  }
}

// largest r in [0, n) with off[r] <= t (off non-decreasing, off[0] <= t)
__device__ inline int64_t row_of(const int64_t* off, int64_t n, int64_t t) {
  int64_t a = 0, b = n - 1;
  while (a < b) {
    const int64_t m = (a + b + 1) >> 1;
    if (off[m] <= t) a = m;
    else b = m - 1;
  }
  return a;
}

template <typename O>
__global__ __launch_bounds__(kBlock) void expand_ranges_kernel(const int64_t* __restrict__ off,
                                                              const int64_t* __restrict__ lo, int64_t ns,
                                                              int64_t total, O* __restrict__ sidx,
                                                              O* __restrict__ bidx) {
  __shared__ int64_t soff[kExpTile + 1];
  __shared__ int64_t rr[2];
  const int64_t t0 = (int64_t)blockIdx.x * kExpTile;
  if (t0 >= total) return;
  const int64_t t1 = t0 + kExpTile < total ? t0 + kExpTile : total;
  if (threadIdx.x == 0) {
    rr[0] = row_of(off, ns, t0);
    rr[1] = row_of(off, ns, t1 - 1);
  }
  __syncthreads();
  const int64_t r0 = rr[0], nr = rr[1] - rr[0] + 1;
  if (nr <= kExpTile) {
    for (int64_t k = threadIdx.x; k < nr; k += blockDim.x) soff[k] = off[r0 + k];
    __syncthreads();
    // each lane expands kExpItems CONSECUTIVE outputs: one search for the
    // first, then a forward walk over the (LDS) range starts, and the lane's
    // outputs leave as whole vectors (a strided layout searched per output)
    const int64_t ta = t0 + (int64_t)threadIdx.x * kExpItems;
    if (ta < t1) {
      int64_t j = row_of(soff, nr, ta);
      int64_t base = lo[r0 + j] - soff[j];
      O sv[kExpItems], bv[kExpItems];
#pragma unroll
      for (int k = 0; k < kExpItems; ++k) {
        const int64_t t = ta + k;
        while (j + 1 < nr && soff[j + 1] <= t) {
          ++j;
          base = lo[r0 + j] - soff[j];
        }
        sv[k] = (O)(r0 + j);
        bv[k] = (O)(base + t);
      }
      if (ta + kExpItems <= t1 && (((uintptr_t)(sidx + ta) | (uintptr_t)(bidx + ta)) & 15) == 0) {
        constexpr int kV = 16 / (int)sizeof(O);   // elements per 16-byte store
        typedef O OV __attribute__((ext_vector_type(kV)));
#pragma unroll
        for (int k = 0; k < kExpItems; k += kV) {
          OV a, b;
#pragma unroll
          for (int q = 0; q < kV; ++q) {
            a[q] = sv[k + q];
            b[q] = bv[k + q];
          }
          *(OV*)(sidx + ta + k) = a;
          *(OV*)(bidx + ta + k) = b;
        }
      } else {
#pragma unroll
        for (int k = 0; k < kExpItems; ++k)
          if (ta + k < t1) {
            sidx[ta + k] = sv[k];
            bidx[ta + k] = bv[k];
          }
      }
    }
  } else {  // many empty ranges inside the tile: search the global offsets
    for (int k = 0; k < kExpItems; ++k) {
      const int64_t t = t0 + threadIdx.x + (int64_t)k * kBlock;
      if (t >= t1) break;
      const int64_t r = row_of(off, ns, t);
      sidx[t] = (O)r;
      bidx[t] = (O)(lo[r] + (t - off[r]));
    }
  }
}

}  // namespace

void sorted_ranges(const void* big, bool key64, int64_t nb, const void* q, const uint8_t* qvalid, int64_t nq,
                   int64_t* lo, int64_t* cnt, const void* fence, int64_t nf, hipStream_t stream) {
  if (nq <= 0) return;
  const unsigned grid = grid_for(nq, kBlock, 1 << 16);
  dispatch(wide{key64}, [&](auto k) {
    using K = type_of<decltype(k)>;
    launch("sorted_ranges", sorted_ranges_kernel<K>, dim3(grid), dim3(kBlock), 0, stream, as<K>(big), nb, as<K>(q),
           qvalid, nq, lo, cnt, as<K>(fence), nf);
  });
}

void expand_ranges(const int64_t* off, const int64_t* lo, int64_t ns, int64_t total, void* sidx, void* bidx,
                   bool out64, hipStream_t stream) {
  if (total <= 0 || ns <= 0) return;
  const unsigned grid = (unsigned)((total + kExpTile - 1) / kExpTile);
  dispatch(wide{out64}, [&](auto o) {
    using O = type_of<decltype(o)>;
    launch("expand_ranges", expand_ranges_kernel<O>, dim3(grid), dim3(kBlock), 0, stream, off, lo, ns, total,
           as<O>(sidx), as<O>(bidx));
  });
}

}  // namespace kern
}  // namespace igloo

// ---- sorted ranges + a second equality key ---------------------------------
// Two-column equi-join whose big side is sorted on the first key (partsupp by
// ps_partkey joined on (partkey, suppkey): TPC-H Q9): after sorted_ranges on
// the first key, each probe row scans its (short) range for the second key.
// Pass 0 counts matches per probe row; pass 1 writes the (probe, build) pairs
// at the exclusive offsets of those counts.
namespace igloo {
namespace kern {
namespace {

// MASKED: big2 is a byte mask over the big side (a filter the big column was
// not compacted by: the join probes the table's own sorted key column) and a
// range row matches where it is set; small2 is unused.
template <typename K2, typename O, bool WRITE, bool MASKED = false>
__global__ __launch_bounds__(kBlock) void sorted_match_kernel(const K2* __restrict__ big2,
                                                             const K2* __restrict__ small2,
                                                             const int64_t* __restrict__ lo,
                                                             const int64_t* __restrict__ cnt, int64_t ns,
                                                             int32_t* __restrict__ counts,
                                                             const int64_t* __restrict__ offsets,
                                                             O* __restrict__ sidx, O* __restrict__ bidx,
                                                             int64_t out_cap, O* __restrict__ first) {
  const uint8_t* __restrict__ mask = reinterpret_cast<const uint8_t*>(big2);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ns; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = lo[i], c = cnt[i];
    const K2 key = MASKED ? K2{} : small2[i];
    int64_t o = WRITE ? offsets[i] : 0;
    int32_t m = 0;
    int64_t f = -1;
    for (int64_t k = 0; k < c; ++k) {
      if (MASKED ? mask[l + k] != 0 : big2[l + k] == key) {
        if (WRITE) {
          // (offsets from a device scan; the outputs sized by a possibly
          // replayed total: never written past it)
          if (o >= 0 && o < out_cap) {
            sidx[o] = (O)i;
            bidx[o] = (O)(l + k);
          }
          ++o;
        }
        if (m == 0) f = l + k;
        ++m;
      }
    }
    if (!WRITE) {
      counts[i] = m;
      // count pass: the first match too (a row with exactly one match -- every
      // row, for a foreign key into a primary key -- needs no write pass)
      if (first) first[i] = (O)f;
    }
  }
}

// the count pass (no offsets yet) exists with 32-bit outputs only
template <typename K2, bool MASKED>
void launch_match(const char* what, const void* big2, const void* small2, const int64_t* lo, const int64_t* cnt,
                  int64_t ns, int32_t* counts, const int64_t* offsets, void* sidx, void* bidx, bool out64,
                  int64_t out_cap, int32_t* first, hipStream_t stream) {
  const dim3 g(grid_for(ns, kBlock, 1 << 16)), b(kBlock);
  if (!offsets) {
    launch(what, sorted_match_kernel<K2, int32_t, false, MASKED>, g, b, 0, stream, as<K2>(big2), as<K2>(small2), lo,
           cnt, ns, counts, nullptr, nullptr, nullptr, 0, first);
    return;
  }
  dispatch(wide{out64}, [&](auto o) {
    using O = type_of<decltype(o)>;
    launch(what, sorted_match_kernel<K2, O, true, MASKED>, g, b, 0, stream, as<K2>(big2), as<K2>(small2), lo, cnt, ns,
           nullptr, offsets, as<O>(sidx), as<O>(bidx), out_cap, nullptr);
  });
}

}  // namespace

void sorted_match(const void* big2, const void* small2, bool key64, const int64_t* lo, const int64_t* cnt,
                  int64_t ns, int32_t* counts, const int64_t* offsets, void* sidx, void* bidx, bool out64,
                  int64_t out_cap, int32_t* first, hipStream_t stream) {
  if (ns <= 0) return;
  dispatch(wide{key64}, [&](auto k) {
    launch_match<type_of<decltype(k)>, false>("sorted_match", big2, small2, lo, cnt, ns, counts, offsets, sidx, bidx,
                                              out64, out_cap, first, stream);
  });
}

void sorted_masked(const uint8_t* mask, const int64_t* lo, const int64_t* cnt, int64_t ns, int32_t* counts,
                   const int64_t* offsets, void* sidx, void* bidx, bool out64, int64_t out_cap, hipStream_t stream) {
  if (ns <= 0) return;
  launch_match<int32_t, true>("sorted_masked", mask, nullptr, lo, cnt, ns, counts, offsets, sidx, bidx, out64, out_cap,
                              nullptr, stream);
}

}  // namespace kern
}  // namespace igloo

// ---- dense range index over a sorted key column -----------------------------
// For a non-decreasing key column whose value span is close to its length
// (partsupp.ps_partkey: 4 rows per key; orders.o_orderkey: 1 of 4 values used)
// a lower-bound table first[k - kmin] = first row with key >= k turns each
// range lookup into two adjacent loads instead of a ~27-step binary search
// whose probes miss the cache when the queries arrive in random key order
// (Q9 probes partsupp in lineitem order: 11 ms searching vs ~1 ms indexed).
// Row i fills the entries between the previous row's key and its own.
//
// That flat table spends 4 bytes per key VALUE, and a lookup fetches a 128-byte
// line of it to learn one entry (orders.o_orderkey at SF100: 2.4 GB for 150M
// rows). Large resident columns (ops/hashing.py dense_index picks the form)
// get a two-level index instead:
//   rank level: one 16-byte entry per 64 key values, {64-bit presence word,
//     number of distinct keys in all earlier entries}: 0.25 B per key value,
//     one load per lookup. present = bit (k - kmin) & 63 of the word;
//     r = rank + popcount(bits below it) = distinct keys < k.
//   starts level (columns with repeated keys): starts[r] = first row of the
//     r-th distinct key, starts[nd] = first row past kmax, so
//     lo = starts[r] (the lower bound for absent keys too) and
//     cnt = present ? starts[r + 1] - starts[r] : 0.
// The four forms: distinct contiguous keys need no table (row = k - kmin);
// distinct keys with holes the rank level alone (row = r); repeated keys
// with no holes the flat table (it IS the starts level under an identity
// rank); repeated keys with holes both levels. The build sets presence bits
// from the run starts (rows whose key differs from the previous row's), scans
// their popcounts and scatters the run starts: no flat table, no gap filling.
namespace igloo {
namespace kern {
namespace {

// Gaps longer than kGapFill are not filled (one lane would serialise them):
// the key's own entry is still written and *long_gap is set, so the caller
// pre-fills the table with -1, rebuilds, and runs the fix-up pass
// (long_gap == null) that searches the entries left at -1.
constexpr int64_t kGapFill = 64;

template <typename K, typename I>
__global__ __launch_bounds__(kBlock) void dense_index_kernel(const K* __restrict__ big, int64_t nb, int64_t kmin,
                                                            int64_t kmax, I* __restrict__ first,
                                                            int32_t* __restrict__ long_gap) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= nb; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t prev = i == 0 ? kmin - 1 : (int64_t)big[i - 1];
    const int64_t cur = i == nb ? kmax + 1 : (int64_t)big[i];
    if (cur == prev) continue;
    int64_t k = cur - prev > kGapFill ? cur : prev + 1;
    if (k != prev + 1) *long_gap = 1;
    // keys outside [kmin, kmax] (a replayed range narrower than the data)
    // never index past the table's kmax - kmin + 2 entries
    const int64_t hi = cur < kmax + 1 ? cur : kmax + 1;
    for (k = k < kmin ? kmin : k; k <= hi; ++k) first[k - kmin] = (I)i;
  }
}

// long-gap fix-up: entries still holding the sentinel get a lower-bound search
// (neighbouring lanes search neighbouring keys, so the probes share cache lines)
template <typename K, typename I>
__global__ __launch_bounds__(kBlock) void dense_fill_kernel(const K* __restrict__ big, int64_t nb, int64_t kmin,
                                                           int64_t span, I sentinel, I* __restrict__ first) {
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k <= span; k += (int64_t)gridDim.x * blockDim.x) {
    if (first[k] != sentinel) continue;
    const int64_t key = kmin + k;
    int64_t a = 0, b = nb;
    while (a < b) {
      const int64_t m = (a + b) >> 1;
      if ((int64_t)big[m] < key) a = m + 1;
      else b = m;
    }
    first[k] = (I)a;
  }
}

template <typename K, typename I>
__global__ __launch_bounds__(kBlock) void dense_ranges_kernel(const I* __restrict__ first, int64_t kmin, int64_t kmax,
                                                             const K* __restrict__ q,
                                                             const uint8_t* __restrict__ qvalid, int64_t nq,
                                                             int64_t* __restrict__ lo_out,
                                                             int64_t* __restrict__ cnt_out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = (int64_t)q[i];
    int64_t lo = 0, c = 0;
    if ((!qvalid || qvalid[i]) && k >= kmin && k <= kmax) {
      lo = (int64_t)first[k - kmin];
      c = (int64_t)first[k - kmin + 1] - lo;
    }
    lo_out[i] = lo;
    cnt_out[i] = c;
  }
}

// ---- the two-level form ----
struct alignas(16) RankEntry {
  uint64_t bits;   // key kmin + 64 * w + b is in the column <=> bit b
  uint32_t rank;   // distinct keys in entries [0, w)
  uint32_t pad;
};
typedef uint32_t RankWords __attribute__((ext_vector_type(4)));

constexpr int kRankChunk = 16;  // build: consecutive rows per lane, their bits merged before the atomic
constexpr int kRankRows = 4;    // lookup: probe rows in flight per lane (two dependent loads each)

// presence bits from the run starts. A lane walks kRankChunk consecutive rows
// and ORs the bits that share a word in a register: sorted keys change word
// rarely, so it issues one or two atomics, not one per row. Keys outside
// [kmin, kmax] (a recorded range narrower than the data) set nothing.
template <typename K>
__global__ __launch_bounds__(kBlock) void rank_bits_kernel(const K* __restrict__ big, int64_t nb, int64_t kmin,
                                                          int64_t kmax, RankEntry* __restrict__ e) {
  const int64_t nchunk = (nb + kRankChunk - 1) / kRankChunk;
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nchunk; c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = c * kRankChunk, i1 = i0 + kRankChunk < nb ? i0 + kRankChunk : nb;
    int64_t prev = i0 > 0 ? (int64_t)big[i0 - 1] : 0;
    int64_t w = -1;
    uint64_t acc = 0;
    for (int64_t i = i0; i < i1; ++i) {
      const int64_t cur = (int64_t)big[i];
      if ((i == 0 || cur != prev) && cur >= kmin && cur <= kmax) {
        const int64_t j = cur - kmin;
        if ((j >> 6) != w) {
          if (acc) atomicOr((unsigned long long*)&e[w].bits, (unsigned long long)acc);
          w = j >> 6;
          acc = 0;
        }
        acc |= uint64_t{1} << (j & 63);
      }
      prev = cur;
    }
    if (acc) atomicOr((unsigned long long*)&e[w].bits, (unsigned long long)acc);
  }
}

__global__ __launch_bounds__(kBlock) void rank_counts_kernel(const RankEntry* __restrict__ e, int64_t nw,
                                                            int32_t* __restrict__ counts) {
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < nw; w += (int64_t)gridDim.x * blockDim.x)
    counts[w] = __popcll(e[w].bits);
}

__global__ __launch_bounds__(kBlock) void rank_finish_kernel(RankEntry* __restrict__ e, int64_t nw,
                                                            const int64_t* __restrict__ off) {
  for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < nw; w += (int64_t)gridDim.x * blockDim.x)
    e[w].rank = (uint32_t)off[w];
}

// (present, r = distinct keys < kmin + j) for j in [0, span); RANKED false:
// every key value present, r = j
template <bool RANKED>
__device__ inline void rank_locate(const RankEntry* __restrict__ e, int64_t j, bool& present, int64_t& r) {
  if (!RANKED) {
    present = true;
    r = j;
    return;
  }
  const RankWords v = *reinterpret_cast<const RankWords*>(e + (j >> 6));   // one 16-byte load: word and rank
  const uint64_t bits = (uint64_t)v.x | ((uint64_t)v.y << 32);
  const int b = (int)(j & 63);
  present = (bits >> b) & 1;
  r = (int64_t)v.z + __popcll(bits & ((uint64_t{1} << b) - 1));
}

// run starts scattered to their rank; the one row (or nb) where the keys pass
// kmax closes the last run. r < nd holds by construction (the bits came from
// the same rows); the test keeps a changed column from writing past starts.
template <typename K, typename S>
__global__ __launch_bounds__(kBlock) void rank_starts_kernel(const K* __restrict__ big, int64_t nb, int64_t kmin,
                                                            int64_t kmax, const RankEntry* __restrict__ e,
                                                            S* __restrict__ starts, int64_t nd) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= nb; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t prev = i > 0 ? (int64_t)big[i - 1] : 0;
    const int64_t cur = i < nb ? (int64_t)big[i] : 0;
    if (i < nb && (i == 0 || cur != prev) && cur >= kmin && cur <= kmax) {
      bool present;
      int64_t r;
      rank_locate<true>(e, cur - kmin, present, r);
      if (r < nd) starts[r] = (S)i;
    }
    if ((i == nb || cur > kmax) && (i == 0 || prev <= kmax)) starts[nd] = (S)i;
  }
}

// The lookups keep kRankRows probe rows per lane in flight: all keys are
// loaded, then all entries, then all starts. Every load is unconditional (a
// row past the end re-reads row nq - 1, a key outside [kmin, kmax] or a NULL
// reads entry 0, starts[r + 1] is clamped to starts[nd]) so the compiler
// batches them instead of branching around and waiting for each.
template <typename K, bool VALID>
__device__ inline void rank_probe_keys(const K* __restrict__ q, const uint8_t* __restrict__ qvalid, int64_t nq,
                                       int64_t t0, int64_t kmin, int64_t kmax, bool (&in)[kRankRows],
                                       bool (&ok)[kRankRows], int64_t (&j)[kRankRows]) {
#pragma unroll
  for (int u = 0; u < kRankRows; ++u) {
    const int64_t i = t0 + (int64_t)u * kBlock + threadIdx.x;
    in[u] = i < nq;
    const int64_t ii = in[u] ? i : nq - 1;
    const int64_t k = (int64_t)q[ii];
    bool v = in[u] && k >= kmin && k <= kmax;
    if (VALID) v = v && qvalid[ii] != 0;
    ok[u] = v;
    j[u] = v ? k - kmin : 0;
  }
}

template <typename K, typename S, bool RANKED, bool STARTS, bool VALID>
__global__ __launch_bounds__(kBlock) void rank_ranges_kernel(const RankEntry* __restrict__ e,
                                                            const S* __restrict__ starts, int64_t nd, int64_t kmin,
                                                            int64_t kmax, const K* __restrict__ q,
                                                            const uint8_t* __restrict__ qvalid, int64_t nq,
                                                            int64_t* __restrict__ lo_out,
                                                            int64_t* __restrict__ cnt_out) {
  constexpr int64_t kTile = (int64_t)kBlock * kRankRows;
  for (int64_t t0 = blockIdx.x * kTile; t0 < nq; t0 += (int64_t)gridDim.x * kTile) {
    bool in[kRankRows], ok[kRankRows], present[kRankRows];
    int64_t j[kRankRows], r[kRankRows], lo[kRankRows], c[kRankRows];
    rank_probe_keys<K, VALID>(q, qvalid, nq, t0, kmin, kmax, in, ok, j);
#pragma unroll
    for (int u = 0; u < kRankRows; ++u) rank_locate<RANKED>(e, j[u], present[u], r[u]);
#pragma unroll
    for (int u = 0; u < kRankRows; ++u) {
      if (STARTS) {
        const int64_t r1 = r[u] < nd ? r[u] + 1 : nd;
        lo[u] = (int64_t)starts[r[u]];
        c[u] = (int64_t)starts[r1] - lo[u];
      } else {
        lo[u] = r[u];
        c[u] = 1;
      }
    }
#pragma unroll
    for (int u = 0; u < kRankRows; ++u) {
      const int64_t i = t0 + (int64_t)u * kBlock + threadIdx.x;
      if (in[u]) {
        lo_out[i] = ok[u] ? lo[u] : 0;
        cnt_out[i] = ok[u] && present[u] ? c[u] : 0;
      }
    }
  }
}

template <typename K, typename S, bool RANKED, bool STARTS, bool VALID>
__global__ __launch_bounds__(kBlock) void rank_unique_kernel(const RankEntry* __restrict__ e,
                                                            const S* __restrict__ starts, int64_t nd, int64_t kmin,
                                                            int64_t kmax, const K* __restrict__ q,
                                                            const uint8_t* __restrict__ qvalid, int64_t nq,
                                                            uint8_t* __restrict__ hit, int32_t* __restrict__ pos) {
  constexpr int64_t kTile = (int64_t)kBlock * kRankRows;
  for (int64_t t0 = blockIdx.x * kTile; t0 < nq; t0 += (int64_t)gridDim.x * kTile) {
    bool in[kRankRows], ok[kRankRows], present[kRankRows];
    int64_t j[kRankRows], r[kRankRows], row[kRankRows];
    rank_probe_keys<K, VALID>(q, qvalid, nq, t0, kmin, kmax, in, ok, j);
#pragma unroll
    for (int u = 0; u < kRankRows; ++u) rank_locate<RANKED>(e, j[u], present[u], r[u]);
#pragma unroll
    for (int u = 0; u < kRankRows; ++u) row[u] = STARTS ? (int64_t)starts[r[u]] : r[u];
#pragma unroll
    for (int u = 0; u < kRankRows; ++u) {
      const int64_t i = t0 + (int64_t)u * kBlock + threadIdx.x;
      if (in[u]) {
        const bool h = ok[u] && present[u];
        hit[i] = h ? 1 : 0;
        pos[i] = h ? (int32_t)row[u] : 0;
      }
    }
  }
}

}  // namespace

void dense_index_build(const void* big, bool key64, int64_t nb, int64_t kmin, int64_t kmax, void* first, bool first64,
                       int32_t* long_gap, hipStream_t stream) {
  const dim3 b(kBlock);
  dispatch(wide{key64}, wide{first64}, [&](auto k, auto i) {
    using K = type_of<decltype(k)>;
    using I = type_of<decltype(i)>;
    if (!long_gap) {  // fix-up pass
      const int64_t span = kmax - kmin + 1;
      const dim3 g(grid_for(span + 1, kBlock, 1 << 16));
      launch("dense_index_build", dense_fill_kernel<K, I>, g, b, 0, stream, as<K>(big), nb, kmin, span, (I)-1,
             as<I>(first));
    } else {
      const dim3 g(grid_for(nb + 1, kBlock, 1 << 16));
      launch("dense_index_build", dense_index_kernel<K, I>, g, b, 0, stream, as<K>(big), nb, kmin, kmax, as<I>(first),
             long_gap);
    }
  });
}

void dense_ranges(const void* first, bool first64, int64_t kmin, int64_t kmax, const void* q, bool key64,
                  const uint8_t* qvalid, int64_t nq, int64_t* lo, int64_t* cnt, hipStream_t stream) {
  if (nq <= 0) return;
  const dim3 g(grid_for(nq, kBlock, 1 << 16)), b(kBlock);
  dispatch(wide{key64}, wide{first64}, [&](auto k, auto i) {
    using K = type_of<decltype(k)>;
    using I = type_of<decltype(i)>;
    launch("dense_ranges", dense_ranges_kernel<K, I>, g, b, 0, stream, as<I>(first), kmin, kmax, as<K>(q), qvalid, nq,
           lo, cnt);
  });
}

void rank_index_bits(const void* big, bool key64, int64_t nb, int64_t kmin, int64_t kmax, void* entries,
                     hipStream_t stream) {
  if (nb <= 0) return;
  const dim3 g(grid_for((nb + kRankChunk - 1) / kRankChunk, kBlock, 1 << 16)), b(kBlock);
  dispatch(wide{key64}, [&](auto k) {
    using K = type_of<decltype(k)>;
    launch("rank_index_bits", rank_bits_kernel<K>, g, b, 0, stream, as<K>(big), nb, kmin, kmax,
           as<RankEntry>(entries));
  });
}

void rank_index_counts(const void* entries, int64_t nwords, int32_t* counts, hipStream_t stream) {
  if (nwords <= 0) return;
  launch("rank_index_counts", rank_counts_kernel, dim3(grid_for(nwords, kBlock, 1 << 16)), dim3(kBlock), 0, stream,
         as<RankEntry>(entries), nwords, counts);
}

void rank_index_finish(void* entries, int64_t nwords, const int64_t* offsets, hipStream_t stream) {
  if (nwords <= 0) return;
  launch("rank_index_finish", rank_finish_kernel, dim3(grid_for(nwords, kBlock, 1 << 16)), dim3(kBlock), 0, stream,
         as<RankEntry>(entries), nwords, offsets);
}

void rank_index_starts(const void* big, bool key64, int64_t nb, int64_t kmin, int64_t kmax, const void* entries,
                       void* starts, bool starts64, int64_t nd, hipStream_t stream) {
  const dim3 g(grid_for(nb + 1, kBlock, 1 << 16)), b(kBlock);
  dispatch(wide{key64}, wide{starts64}, [&](auto k, auto s) {
    using K = type_of<decltype(k)>;
    using S = type_of<decltype(s)>;
    launch("rank_index_starts", rank_starts_kernel<K, S>, g, b, 0, stream, as<K>(big), nb, kmin, kmax,
           as<RankEntry>(entries), as<S>(starts), nd);
  });
}

void rank_ranges(const void* entries, const void* starts, bool starts64, int64_t nd, int64_t kmin, int64_t kmax,
                 const void* q, bool key64, const uint8_t* qvalid, int64_t nq, int64_t* lo, int64_t* cnt,
                 hipStream_t stream) {
  if (nq <= 0) return;
  const dim3 g(grid_for(nq, kBlock * kRankRows, 1 << 16)), b(kBlock);
  pick(qvalid != nullptr, [&](auto v) {
    dispatch(wide{key64}, wide{starts64}, entries != nullptr, starts != nullptr,
             [&](auto k, auto s, auto rk, auto st) {
               using K = type_of<decltype(k)>;
               using S = type_of<decltype(s)>;
               constexpr bool kRanked = decltype(rk)::value, kStarts = decltype(st)::value;
               constexpr bool kValid = decltype(v)::value;
               launch("rank_ranges", rank_ranges_kernel<K, S, kRanked, kStarts, kValid>, g, b, 0, stream,
                      as<RankEntry>(entries), as<S>(starts), nd, kmin, kmax, as<K>(q), qvalid, nq, lo, cnt);
             });
  });
}

void rank_unique(const void* entries, const void* starts, bool starts64, int64_t nd, int64_t kmin, int64_t kmax,
                 const void* q, bool key64, const uint8_t* qvalid, int64_t nq, uint8_t* hit, int32_t* pos,
                 hipStream_t stream) {
  if (nq <= 0) return;
  const dim3 g(grid_for(nq, kBlock * kRankRows, 1 << 16)), b(kBlock);
  pick(qvalid != nullptr, [&](auto v) {
    dispatch(wide{key64}, wide{starts64}, entries != nullptr, starts != nullptr,
             [&](auto k, auto s, auto rk, auto st) {
               using K = type_of<decltype(k)>;
               using S = type_of<decltype(s)>;
               constexpr bool kRanked = decltype(rk)::value, kStarts = decltype(st)::value;
               constexpr bool kValid = decltype(v)::value;
               launch("rank_unique", rank_unique_kernel<K, S, kRanked, kStarts, kValid>, g, b, 0, stream,
                      as<RankEntry>(entries), as<S>(starts), nd, kmin, kmax, as<K>(q), qvalid, nq, hit, pos);
             });
  });
}

}  // namespace kern
}  // namespace igloo

// ---- EXISTS over a sorted range with a column comparison ----------------------
// Semi / anti join whose residual compares one column of each side
// (Q21: EXISTS (l2.l_orderkey = l1.l_orderkey AND l2.l_suppkey <> l1.l_suppkey)):
// hit[i] = any k in [lo[i], lo[i]+cnt[i]) with big2[k] OP small2[i], scanned
// in place instead of expanding every pair and gathering both columns.
namespace igloo {
namespace kern {
namespace {
// mask (optional): only the big rows set in it exist (a filtered big side
// searched in place, exec/joins.py _in_place_semi); op 6: any such row
template <typename K2>
__global__ __launch_bounds__(kBlock) void sorted_exists_kernel(const K2* __restrict__ big2,
                                                              const K2* __restrict__ small2,
                                                              const int64_t* __restrict__ lo,
                                                              const int64_t* __restrict__ cnt, int64_t ns, int op,
                                                              const uint8_t* __restrict__ mask,
                                                              uint8_t* __restrict__ hit) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ns; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t l = lo[i], c = cnt[i];
    const K2 v = op == 6 ? K2{} : small2[i];
    bool any = false;
    for (int64_t k = 0; k < c && !any; ++k) {
      if (mask && !mask[l + k]) continue;
      const K2 b = op == 6 ? K2{} : big2[l + k];
      switch (op) {
        case 0: any = b == v; break;
        case 1: any = b != v; break;
        case 2: any = b < v; break;
        case 3: any = b <= v; break;
        case 4: any = b > v; break;
        case 5: any = b >= v; break;
        default: any = true; break;
      }
    }
    hit[i] = any;
  }
}
}  // namespace

void sorted_exists(const void* big2, const void* small2, bool key64, const int64_t* lo, const int64_t* cnt,
                   int64_t ns, int op, const uint8_t* mask, uint8_t* hit, hipStream_t stream) {
  if (ns <= 0) return;
  const dim3 g(grid_for(ns, kBlock, 1 << 16)), b(kBlock);
  dispatch(wide{key64}, [&](auto k) {
    using K2 = type_of<decltype(k)>;
    launch("sorted_exists", sorted_exists_kernel<K2>, g, b, 0, stream, as<K2>(big2), as<K2>(small2), lo, cnt, ns, op,
           mask, hit);
  });
}
}  // namespace kern
}  // namespace igloo

// ---- lookups into UNIQUE sorted keys ----------------------------------------
// A search into a key column known to hold distinct values (a primary key,
// ops/hashing.py key_unique) pairs every probe row with at most one row:
// hit[i] (0/1) and pos[i] (int32 row, 0 on a miss) replace the (lo, cnt)
// int64 pair -- 5 instead of 16 output bytes per probe row, and no compare /
// narrowing pass over them afterwards (exec/joins.py _unique_pairs).
namespace igloo {
namespace kern {
namespace {

template <typename K>
__global__ __launch_bounds__(kBlock) void unique_search_kernel(const K* __restrict__ big, int64_t nb,
                                                              const K* __restrict__ q,
                                                              const uint8_t* __restrict__ qvalid, int64_t nq,
                                                              uint8_t* __restrict__ hit, int32_t* __restrict__ pos,
                                                              const K* __restrict__ fence, int64_t nf) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
    if (qvalid && !qvalid[i]) {
      hit[i] = 0;
      pos[i] = 0;
      continue;
    }
    const K key = q[i];
    int64_t a = 0, b = nb;
    if (fence) {
      int64_t fa = 0, fb = nf;
      while (fa < fb) {
        const int64_t m = (fa + fb) >> 1;
        if (fence[m] < key) fa = m + 1;
        else fb = m;
      }
      a = fa > 0 ? (fa - 1) * kFence : 0;
      b = fa * kFence < nb ? fa * kFence : nb;
    }
    while (a < b) {
      const int64_t m = (a + b) >> 1;
      if (big[m] < key) a = m + 1;
      else b = m;
    }
    const bool h = a < nb && big[a] == key;
    hit[i] = h ? 1 : 0;
    pos[i] = h ? (int32_t)a : 0;
  }
}

template <typename K, typename I>
__global__ __launch_bounds__(kBlock) void unique_dense_kernel(const I* __restrict__ first, int64_t kmin, int64_t kmax,
                                                             const K* __restrict__ q,
                                                             const uint8_t* __restrict__ qvalid, int64_t nq,
                                                             uint8_t* __restrict__ hit, int32_t* __restrict__ pos) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nq; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = (int64_t)q[i];
    int64_t lo = 0;
    bool h = false;
    if ((!qvalid || qvalid[i]) && k >= kmin && k <= kmax) {
      lo = (int64_t)first[k - kmin];
      h = (int64_t)first[k - kmin + 1] > lo;
    }
    hit[i] = h ? 1 : 0;
    pos[i] = h ? (int32_t)lo : 0;
  }
}

}  // namespace

void unique_lookup(const void* big, bool key64, int64_t nb, const void* first, bool first64, int64_t kmin,
                   int64_t kmax, const void* q, const uint8_t* qvalid, int64_t nq, uint8_t* hit, int32_t* pos,
                   const void* fence, int64_t nf, hipStream_t stream) {
  if (nq <= 0) return;
  const dim3 g(grid_for(nq, kBlock, 1 << 16)), b(kBlock);
  dispatch(wide{key64}, wide{first64}, [&](auto k, auto i) {
    using K = type_of<decltype(k)>;
    using I = type_of<decltype(i)>;
    if (first) {
      launch("unique_lookup", unique_dense_kernel<K, I>, g, b, 0, stream, as<I>(first), kmin, kmax, as<K>(q), qvalid,
             nq, hit, pos);
    } else {
      launch("unique_lookup", unique_search_kernel<K>, g, b, 0, stream, as<K>(big), nb, as<K>(q), qvalid, nq, hit, pos,
             as<K>(fence), nf);
    }
  });
}

}  // namespace kern
}  // namespace igloo
