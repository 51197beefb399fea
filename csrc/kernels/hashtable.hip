// GPU hash tables for equi-joins and GROUP BY.
//
// Replaces the reference's HashJoinExec build/probe, which keys a
// HashMap<Vec<u8>, Vec<RecordBatch>> on Debug-formatted key bytes and probes
// row by row (reference crates/engine/src/operators/hash_join.rs:101-128,
// :141-203), and DataFusion's AggregateExec group table.
//
// Layout (struct-of-arrays, one HBM line per probe in the common case):
//   hashed mode: tkeys[cap] int64 (kEmptyKey = empty) + thead[cap] int32,
//                open addressing with linear probing, cap = pow2 >= 2n. The
//                key that equals kEmptyKey lives in one reserved slot, index
//                cap, outside the probed range: every per-slot array of a
//                hashed table has cap + 1 entries, and tkeys[cap] stays
//                kEmptyKey, so that slot "holds" the key from the start;
//   direct mode: when the key domain [kmin, kmin+cap) is dense enough the
//                key itself is the slot (a perfect hash): no key array, no
//                probing, one random read per probe row. TPC-H keys are
//                dense integers, so most joins take this path.
// Every slot's head row (thead, one atomicExch per build row) serves unique
// (PK) builds. A build with duplicate keys adds a CSR layout: per-slot counts,
// an exclusive scan into cstart[cap+1] and a scatter of the row ids into
// crows[n], so a multi-match probe reads one contiguous run instead of
// pointer-chasing a next[] chain through HBM. Row ids (thead, crows, cstart,
// probe outputs) are int32 below 2^31 build rows and int64 above (R).
//
// A join table reaches this file as one JoinTableRef (kernels.h) and its
// kernels as one TableView<R>; the file runs: helpers, build, probe, hit-bit
// probes, GROUP BY, host entry points.
#include "common.h"
#include "kernels.h"
#include "launch.h"

#include <cmath>
#include <cstdint>
#include <string>

namespace igloo {
namespace kern {

namespace {

// ---- helpers -----------------------------------------------------------------
constexpr int kMaxGrid = 256 * 8 * 16;  // 32768 blocks: every CU gets many waves of random loads

// A JoinTableRef as the kernels see it: typed pointers (R: the row-id type)
// and the scalars the slot arithmetic needs. W: the build's view, which
// writes keys, heads and filter bits. Kernels take it by value next to their
// __restrict__ row streams (keys, valid, outputs): every store of a probe goes
// through one of those, so the table's loads need no noalias of their own.
template <typename R, bool W = false>
struct TableView {
  template <typename T> using ptr = std::conditional_t<W, T*, const T*>;
  ptr<int64_t> tkeys;
  ptr<R> thead;
  const R* cstart;
  const R* crows;
  ptr<uint32_t> bits;   // null: no filter, or a probe that does not use it
  int64_t cap, kmin;
  uint64_t bmask;
};

template <typename R, bool W = false>
TableView<R, W> view(const JoinTableRef& t, bool use_filter = true) {
  return {t.tkeys, as<R>(t.thead), as<R>(t.cstart), as<R>(t.crows), use_filter ? t.bits : nullptr,
          t.cap,   t.kmin,         t.bmask};
}

// The exact membership bitmap of a direct table over [kmin, kmin + cap), all
// the bitmap probes read of one (fold: probe_fold_build's scratch, or null)
struct BitmapView {
  const uint32_t* bits;
  const uint32_t* fold;
  int64_t cap, kmin;
};

template <typename K>
__device__ inline bool load_key(const K* keys, const uint8_t* valid, int64_t i, int64_t* out) {
  if (valid && !valid[i]) return false;
  *out = (int64_t)keys[i];
  return true;
}

// First slot of `k`'s probe chain (hashed mode). A key equal to kEmptyKey
// cannot be told from an empty slot, so it starts (and ends: tkeys[cap] is
// never claimed and compares equal to it) at the reserved slot past the table.
__device__ inline int64_t home_slot(int64_t mask, int64_t k) {
  return k == kEmptyKey ? mask + 1 : (int64_t)(mix64((uint64_t)k) & (uint64_t)mask);
}

// Find the slot holding `k` (hashed mode); -1 when absent (the reserved slot
// for k == kEmptyKey: its per-slot entries are empty when no row had the key).
__device__ inline int64_t find_slot(const int64_t* __restrict__ tkeys, int64_t mask, int64_t k) {
  int64_t slot = home_slot(mask, k);
  for (;;) {
    int64_t tk = tkeys[slot];
    if (tk == k) return slot;
    if (tk == kEmptyKey) return -1;
    slot = (slot + 1) & mask;
  }
}
template <typename R>
__device__ inline int64_t find_slot(const TableView<R>& t, int64_t k) {
  return find_slot(t.tkeys, t.cap - 1, k);
}

// Insert-or-find `k` (hashed mode); returns the slot and whether the key
// already existed.
// A slot's key is read before it is claimed: a key already in the table (every
// row of a low-cardinality GROUP BY -- Q22's 7 country codes over 4M rows,
// which serialised on 7 words as one CAS per row) costs one load, and only an
// empty slot takes the CAS. Keys are never removed or changed once set, so a
// stale read can only show EMPTY, which the CAS then settles -- the read may
// therefore be a plain (L1-cached) load: hot slots are served per CU instead
// of queueing on one L2 line.
__device__ inline int64_t insert_slot(int64_t* __restrict__ tkeys, int64_t mask, int64_t k, bool* existed) {
  int64_t slot = home_slot(mask, k);
  for (;;) {
    const int64_t cur = tkeys[slot];
    if (cur == k) { *existed = true; return slot; }
    if (cur == kEmptyKey) {
      unsigned long long prev = atomicCAS((unsigned long long*)&tkeys[slot], (unsigned long long)kEmptyKey,
                                          (unsigned long long)k);
      if ((int64_t)prev == kEmptyKey) { *existed = false; return slot; }
      if ((int64_t)prev == k) { *existed = true; return slot; }
    }
    slot = (slot + 1) & mask;
  }
}

// Optional 1-hash Bloom filter over the build keys (<= 4 MB, so it stays in a
// XCD's L2): a selective probe (most probe keys absent) answers from L2 and
// never touches the HBM-sized table.
// Bloom bit of key k. With kExactBits set in bmask (direct-mapped tables whose
// key span fits the bitmap, ops/hashing.py JoinTable) the "filter" is an exact
// membership bitmap indexed by k - kmin: no false positives, so a probe reads
// the table only for keys that are present. Callers range-check k first.
constexpr uint64_t kExactBits = 1ull << 63;
__device__ inline uint64_t bloom_bit(int64_t k, uint64_t bmask, int64_t kmin) {
  return (bmask & kExactBits) ? (uint64_t)(k - kmin) : ((mix64((uint64_t)k) >> 7) & bmask);
}

__device__ inline int32_t atomic_add(int32_t* p, int32_t v) { return atomicAdd(p, v); }
__device__ inline int64_t atomic_add(int64_t* p, int64_t v) {
  return (int64_t)atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}
__device__ inline int32_t atomic_exch(int32_t* p, int32_t v) { return atomicExch(p, v); }
__device__ inline int64_t atomic_exch(int64_t* p, int64_t v) {
  return (int64_t)atomicExch(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// ---- build -------------------------------------------------------------------
// One launch for everything join_build expects initialised: thead = -1,
// tkeys = kEmptyKey (hashed tables), bits = 0, dups = 0 (cap: entries of
// thead and tkeys, a hashed table's reserved slot included). A segment is an
// array of 4-byte words whose fill repeats every 8 bytes (lo, hi): 16-byte
// stores over its whole chunks, word stores for the up to three words left.
struct FillSeg {
  uint32_t* p;
  int64_t words;
  uint32_t lo, hi;
};

__global__ __launch_bounds__(kBlock) void join_table_init_kernel(FillSeg a, FillSeg b, FillSeg c,
                                                                unsigned long long* __restrict__ dups) {
  const int64_t na = a.words >> 2, nb = b.words >> 2, nc = c.words >> 2;
  const int64_t total = na + nb + nc;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    uint32_t* p = a.p;
    uint32_t lo = a.lo, hi = a.hi;
    int64_t j = i;
    if (j >= na) {
      j -= na;
      p = b.p, lo = b.lo, hi = b.hi;
      if (j >= nb) {
        j -= nb;
        p = c.p, lo = c.lo, hi = c.hi;
      }
    }
    reinterpret_cast<uint4*>(p)[j] = make_uint4(lo, hi, lo, hi);
  }
  if (blockIdx.x == 0 && threadIdx.x < 3) {
    const FillSeg s = threadIdx.x == 0 ? a : threadIdx.x == 1 ? b : c;
    for (int64_t w = s.words & ~(int64_t)3; w < s.words; ++w) s.p[w] = (w & 1) ? s.hi : s.lo;
  }
  if (blockIdx.x == 0 && threadIdx.x == 3) *dups = 0ULL;
}

template <typename K, bool DIRECT, typename R>
__global__ __launch_bounds__(kBlock) void join_build_kernel(const K* __restrict__ keys, const uint8_t* __restrict__ valid,
                                                           int64_t n, TableView<R, true> t, unsigned long long* dups) {
  const int64_t mask = t.cap - 1;
  unsigned long long local_dups = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t k;
    if (!load_key(keys, valid, i, &k)) continue;
    int64_t slot;
    if (DIRECT) {
      slot = k - t.kmin;
      // a key outside the span only occurs under a replayed key range that the
      // end-of-query check will reject (ops/_lib.py Speculation): stay in bounds
      if ((uint64_t)slot >= (uint64_t)t.cap) continue;
    } else {
      bool existed;
      slot = insert_slot(t.tkeys, mask, k, &existed);
    }
    const R old = atomic_exch(&t.thead[slot], (R)i);
    local_dups += old != (R)-1;
    if (t.bits) {
      const uint64_t bb = bloom_bit(k, t.bmask, t.kmin);
      atomicOr(&t.bits[bb >> 5], 1u << (bb & 31));
    }
  }
  // one atomic per wave for the duplicate counter
  for (int off = kWave / 2; off > 0; off >>= 1) local_dups += __shfl_xor(local_dups, off, kWave);
  if (lane_id() == 0 && local_dups) atomicAdd(dups, local_dups);
}

// slot of build row i (its key is in the table), -1 for a NULL key
template <typename K, bool DIRECT, typename R>
__device__ inline int64_t build_slot(const K* keys, const uint8_t* valid, int64_t i, const TableView<R>& t) {
  int64_t k;
  if (!load_key(keys, valid, i, &k)) return -1;
  if (DIRECT) {
    const int64_t s = k - t.kmin;
    return (uint64_t)s < (uint64_t)t.cap ? s : -1;
  }
  return find_slot(t, k);
}

// CSR pass 1: rows per slot (cnt zeroed by the caller)
template <typename K, bool DIRECT, typename R>
__global__ __launch_bounds__(kBlock) void join_csr_count_kernel(const K* __restrict__ keys,
                                                               const uint8_t* __restrict__ valid, int64_t n,
                                                               TableView<R> t, R* __restrict__ cnt) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = build_slot<K, DIRECT>(keys, valid, i, t);
    if (s >= 0) atomic_add(&cnt[s], (R)1);
  }
}

// CSR pass 2 (t.cstart = exclusive scan of cnt): every row claims a position
// of its slot's run by counting cnt back down; crows: the table's, written here
template <typename K, bool DIRECT, typename R>
__global__ __launch_bounds__(kBlock) void join_csr_scatter_kernel(const K* __restrict__ keys,
                                                                 const uint8_t* __restrict__ valid, int64_t n,
                                                                 TableView<R> t, R* __restrict__ cnt,
                                                                 R* __restrict__ crows) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = build_slot<K, DIRECT>(keys, valid, i, t);
    if (s < 0) continue;
    const R pos = atomic_add(&cnt[s], (R)-1) - 1;
    crows[(int64_t)t.cstart[s] + pos] = (R)i;
  }
}

// ---- probe -------------------------------------------------------------------
// slot holding probe row j's key, -1 when the key is NULL, outside the span,
// filtered out by the bitmap or (hashed) absent; a direct slot may be empty
template <typename K, bool DIRECT, typename R>
__device__ inline int64_t probe_slot(const K* keys, const uint8_t* valid, int64_t j, const TableView<R>& t) {
  int64_t k;
  if (!load_key(keys, valid, j, &k)) return -1;
  if (DIRECT && (k - t.kmin < 0 || k - t.kmin >= t.cap)) return -1;
  if (t.bits) {
    const uint64_t b = bloom_bit(k, t.bmask, t.kmin);
    if (!((t.bits[b >> 5] >> (b & 31)) & 1u)) return -1;
  }
  if (DIRECT) return k - t.kmin;
  return find_slot(t, k);
}

// counts[j] = number of build matches of probe row j; first[j] = one match or
// -1; build_matched[r] = 1 for every matched build row. t.cstart / t.crows:
// the CSR runs of a duplicate-key build (null: unique build, thead only).
template <typename K, bool DIRECT, typename R>
__global__ __launch_bounds__(kBlock) void join_probe_kernel(const K* __restrict__ keys, const uint8_t* __restrict__ valid,
                                                           int64_t m, TableView<R> t, int32_t* __restrict__ counts,
                                                           R* __restrict__ first, uint8_t* __restrict__ build_matched) {
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = probe_slot<K, DIRECT>(keys, valid, j, t);
    R h = (R)-1;
    int64_t a = 0, e = 0;
    if (s >= 0) {
      if (t.cstart) {
        a = t.cstart[s];
        e = t.cstart[s + 1];
        if (a < e) h = t.crows[a];
      } else {
        h = t.thead[s];
        e = h >= 0;
      }
    }
    if (first) first[j] = h;
    if (counts) counts[j] = (int32_t)(e - a);
    if (build_matched) {
      if (t.cstart) {
        for (int64_t r = a; r < e; ++r) build_matched[t.crows[r]] = 1;
      } else if (h >= 0) {
        build_matched[h] = 1;
      }
    }
  }
}

// Batched head lookup of N probe rows per lane: every key load, then every
// validity load, then every filter-bit load, then every table load is issued
// before any result is used, so a lane keeps N misses in flight (a
// row-at-a-time dependent chain left the 600M-row lineitem probes at ~10% of
// HBM bandwidth, profiles/r3_sf100_pmc_roofline.txt). With an exact membership
// bitmap the bit IS the answer and the table need not be read at all
// (need_head false). Rows at or past m are skipped (h = -1).
//
// All loads are unconditional (indices clamped into range, results selected
// afterwards): a load under a per-lane condition compiles to a branch whose
// merge waits for it, which would serialise the batch again.
template <typename K, bool DIRECT, typename R, int N>
__device__ inline void probe_heads(const K* __restrict__ keys, const uint8_t* __restrict__ valid, int64_t m,
                                   const int64_t (&row)[N], const TableView<R>& t, bool need_head, int64_t (&h)[N]) {
  int64_t k[N], rc[N];
  bool ok[N];
#pragma unroll
  for (int r = 0; r < N; ++r) {
    rc[r] = row[r] < m ? row[r] : m - 1;
    k[r] = (int64_t)keys[rc[r]];
  }
  uint8_t vb[N];
#pragma unroll
  for (int r = 0; r < N; ++r) vb[r] = 1;
  if (valid) {
#pragma unroll
    for (int r = 0; r < N; ++r) vb[r] = valid[rc[r]];
  }
#pragma unroll
  for (int r = 0; r < N; ++r) {
    ok[r] = row[r] < m && vb[r];
    if (DIRECT) ok[r] = ok[r] && k[r] - t.kmin >= 0 && k[r] - t.kmin < t.cap;
  }
  if (t.bits) {
    uint32_t w[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
      // exact bitmaps index by k - kmin: out-of-span keys (ok false) read bit 0
      const uint64_t b = ok[r] || !(t.bmask & kExactBits) ? bloom_bit(k[r], t.bmask, t.kmin) : 0;
      w[r] = t.bits[b >> 5] >> (b & 31);
    }
#pragma unroll
    for (int r = 0; r < N; ++r) ok[r] = ok[r] && (w[r] & 1u);
  }
  if (!need_head) {
#pragma unroll
    for (int r = 0; r < N; ++r) h[r] = ok[r] ? 0 : -1;
    return;
  }
  if (DIRECT) {
    R x[N];
#pragma unroll
    for (int r = 0; r < N; ++r) x[r] = t.thead[ok[r] ? k[r] - t.kmin : 0];
#pragma unroll
    for (int r = 0; r < N; ++r) h[r] = ok[r] ? x[r] : -1;
  } else {
    // first slot of every row in flight together; collisions walk on serially
    const int64_t mask = t.cap - 1;
    int64_t slot[N], tk[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
      slot[r] = home_slot(mask, k[r]);
      tk[r] = t.tkeys[slot[r]];
    }
#pragma unroll
    for (int r = 0; r < N; ++r) {
      while (ok[r] && tk[r] != k[r] && tk[r] != kEmptyKey) {
        slot[r] = (slot[r] + 1) & mask;
        tk[r] = t.tkeys[slot[r]];
      }
      ok[r] = ok[r] && tk[r] == k[r];
    }
    R x[N];
#pragma unroll
    for (int r = 0; r < N; ++r) x[r] = t.thead[ok[r] ? slot[r] : 0];
#pragma unroll
    for (int r = 0; r < N; ++r) h[r] = ok[r] ? x[r] : -1;
  }
}

// first-match probe, direct-mapped table: probe_heads over 4 rows per lane, a
// grid stride apart (600M-row lineitem probes were latency-bound on one
// dependent chain per lane)
constexpr int kProbeRows = 4;

template <typename K, typename R>
__global__ __launch_bounds__(kBlock) void join_probe_first_direct_kernel(const K* __restrict__ keys,
                                                                        const uint8_t* __restrict__ valid, int64_t m,
                                                                        TableView<R> t, R* __restrict__ first) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j0 < m; j0 += stride * kProbeRows) {
    int64_t row[kProbeRows], h[kProbeRows];
#pragma unroll
    for (int r = 0; r < kProbeRows; ++r) row[r] = j0 + r * stride;
    probe_heads<K, true, R, kProbeRows>(keys, valid, m, row, t, true, h);
#pragma unroll
    for (int r = 0; r < kProbeRows; ++r)
      if (row[r] < m) first[row[r]] = (R)h[r];
  }
}

// every (probe row, build row) match at offsets[j] (exclusive scan of counts)
template <typename K, bool DIRECT, typename R>
__global__ __launch_bounds__(kBlock) void join_expand_kernel(const K* __restrict__ keys, const uint8_t* __restrict__ valid,
                                                            int64_t m, TableView<R> t,
                                                            const int64_t* __restrict__ offsets,
                                                            int32_t* __restrict__ out_probe, R* __restrict__ out_build,
                                                            int64_t out_cap) {
  // out_cap: pairs the outputs hold (sized by a possibly replayed total):
  // writes past it are dropped; the end-of-query check rejects the run
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < m; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = probe_slot<K, DIRECT>(keys, valid, j, t);
    if (s < 0) continue;
    int64_t o = offsets[j];
    if (t.cstart) {
      const int64_t e = t.cstart[s + 1];
      for (int64_t r = t.cstart[s]; r < e && o < out_cap; ++r, ++o) {
        out_probe[o] = (int32_t)j;
        out_build[o] = t.crows[r];
      }
    } else {
      const R h = t.thead[s];
      if (h >= 0 && o < out_cap) {
        out_probe[o] = (int32_t)j;
        out_build[o] = h;
      }
    }
  }
}

// ---- hit-bit probes: probe + compaction in two passes --------------------------
// First-match probes whose result is a row selection (inner join on a unique
// build side, semi / anti joins): instead of writing first[] for every probe
// row and compacting it (first: 4 B/row written, compared, flag-compacted:
// ~15 B of traffic per probe row for a 600M-row lineitem probe), pass 1
// writes one hit bit per row and a count per 8192-row tile; pass 2 (after an
// exclusive scan of the tile counts) re-probes only the hit rows and writes
// (probe row, build row) at their final positions, in row order.
constexpr int kHitTile = 8192;                 // rows per tile
constexpr int kHitWords = kHitTile / kWave;    // 64-bit hit words per tile (128)
constexpr int kHitBatch = 8;                   // rows per lane of one probe_heads batch
// probe_write: tiles with at most this many hits list them in LDS and give
// every lane whole hits (denser tiles walk their hit words)
constexpr int kSparseHits = 2048;
// the bitmap probes: every lane takes 4 consecutive rows per step
constexpr int kBitsRows = 4;
constexpr int kBitsSteps = kHitTile / (kBlock * kBitsRows);   // 8

// 4 consecutive keys (16-byte aligned) in one or two 16-byte loads
__device__ inline void load4(const int32_t* p, int32_t (&k)[4]) {
  const int4 v = *reinterpret_cast<const int4*>(p);
  k[0] = v.x;
  k[1] = v.y;
  k[2] = v.z;
  k[3] = v.w;
}
__device__ inline void load4(const int64_t* p, int64_t (&k)[4]) {
  const longlong2 a = *reinterpret_cast<const longlong2*>(p);
  const longlong2 b = *reinterpret_cast<const longlong2*>(p + 2);
  k[0] = a.x;
  k[1] = a.y;
  k[2] = b.x;
  k[3] = b.y;
}

// 4 rows from r0 on, rows past m masked out: keys, validity bytes (vb) and
// the mask of rows below m
template <typename K>
__device__ inline uint32_t load4_guarded(const K* __restrict__ keys, const uint8_t* __restrict__ valid, int64_t r0,
                                         int64_t m, K (&k)[kBitsRows], uint32_t& vb) {
  if (r0 + kBitsRows <= m) {
    load4(keys + r0, k);
    vb = valid ? *reinterpret_cast<const uint32_t*>(valid + r0) : 0x01010101u;
    return 0xfu;
  }
  uint32_t in = 0;
  vb = 0;
#pragma unroll
  for (int j = 0; j < kBitsRows; ++j) {
    const bool here = r0 + j < m;
    k[j] = here ? keys[r0 + j] : K(0);
    if (here && (!valid || valid[r0 + j])) vb |= 1u << (8 * j);
    in |= (here ? 1u : 0u) << j;
  }
  return in;
}

// rows 4*lane .. 4*lane+3 of a wave's 256 are bits 4*(lane%16) .. +3 of word
// lane/16: OR the 16 nibbles of each lane group together (every lane of the
// group gets the word)
__device__ inline unsigned long long nibbles_to_word(uint32_t nib, int lane) {
  unsigned long long w = (unsigned long long)nib << (4 * (lane & 15));
  w |= __shfl_xor(w, 1, kWave);
  w |= __shfl_xor(w, 2, kWave);
  w |= __shfl_xor(w, 4, kWave);
  w |= __shfl_xor(w, 8, kWave);
  return w;
}

// tile_counts[t] = the hits of a tile that a workgroup of WAVES waves shares:
// every wave's count (the same in all its lanes) through LDS, summed by thread 0
template <int WAVES>
__device__ inline void store_tile_count(int64_t wave_cnt, int64_t* __restrict__ tile_counts, int64_t t) {
  __shared__ int64_t red[WAVES];
  if (lane_id() == 0) red[threadIdx.x / kWave] = wave_cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t s = 0;
    for (int w = 0; w < WAVES; ++w) s += red[w];
    tile_counts[t] = s;
  }
  __syncthreads();
}

template <typename K, bool DIRECT, typename R>
__global__ __launch_bounds__(kBlock) void probe_hits_kernel(const K* __restrict__ keys, const uint8_t* __restrict__ valid,
                                                           int64_t m, TableView<R> t, bool negate,
                                                           unsigned long long* __restrict__ words,
                                                           int64_t* __restrict__ tile_counts) {
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tiles = (m + kHitTile - 1) / kHitTile;
  // a direct table with an exact bitmap: bit set <=> key present
  const bool need_head = !(DIRECT && t.bits && (t.bmask & kExactBits));
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int64_t cnt = 0;
    for (int it0 = 0; it0 < kHitTile / kBlock; it0 += kHitBatch) {
      int64_t row[kHitBatch];
      int64_t h[kHitBatch];
#pragma unroll
      for (int r = 0; r < kHitBatch; ++r) row[r] = tile * kHitTile + (int64_t)(it0 + r) * kBlock + threadIdx.x;
      probe_heads<K, DIRECT, R, kHitBatch>(keys, valid, m, row, t, need_head, h);
#pragma unroll
      for (int r = 0; r < kHitBatch; ++r) {
        const bool hit = row[r] < m && ((h[r] >= 0) != negate);
        const unsigned long long b = __ballot(hit);
        if (lane == 0 && tile * kHitTile + (int64_t)(it0 + r) * kBlock + wave * kWave < m)
          words[tile * kHitWords + (it0 + r) * kWavesPerBlock + wave] = b;
        cnt += __popcll(b);
      }
    }
    store_tile_count<kWavesPerBlock>(cnt, tile_counts, tile);
  }
}

template <typename K, bool DIRECT, typename R, typename O>
__global__ __launch_bounds__(kBlock) void probe_write_kernel(const K* __restrict__ keys, const uint8_t* __restrict__ valid,
                                                            int64_t m, TableView<R> t,
                                                            const unsigned long long* __restrict__ words,
                                                            const int64_t* __restrict__ tile_off,
                                                            O* __restrict__ out_probe, R* __restrict__ out_build,
                                                            int64_t out_cap) {
  __shared__ int64_t woff[kHitWords];
  __shared__ int64_t scratch[kWavesPerBlock + 1];
  __shared__ uint16_t hits[kSparseHits];
  t.bits = nullptr;   // the hit rows already passed the filter: a constant, so probe_heads compiles without it
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tiles = (m + kHitTile - 1) / kHitTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // a tile without hits (its offset equals the next one's): nothing to
    // load, scan or write (selective probes: most tiles)
    if ((tile + 1 < tiles ? tile_off[tile + 1] : out_cap) <= tile_off[tile]) continue;
    const int64_t nrows = m - tile * kHitTile < kHitTile ? m - tile * kHitTile : kHitTile;
    const int nwords = (int)((nrows + kWave - 1) / kWave);
    const unsigned long long w0 = threadIdx.x < nwords ? words[tile * kHitWords + threadIdx.x] : 0ULL;
    int64_t total;
    const int64_t ex = block_exclusive_scan((int64_t)__popcll(w0), scratch, &total);
    if (threadIdx.x < kHitWords) woff[threadIdx.x] = ex;
    __syncthreads();
    if (total && total <= kSparseHits) {
      // a sparse tile: its hit rows listed in LDS first (in row order: the
      // list index IS the output offset inside the tile), then every lane
      // takes whole hits -- the work follows the hits, not the 8192 rows
      const int64_t base = tile_off[tile];
      if (threadIdx.x < nwords) {
        unsigned long long w = w0;
        int o = (int)ex;
        while (w) {
          const int b = __ffsll((long long)w) - 1;
          hits[o++] = (uint16_t)(threadIdx.x * kWave + b);
          w &= w - 1ULL;
        }
      }
      __syncthreads();
      for (int64_t i0 = 0; i0 < total; i0 += (int64_t)kBlock * kHitBatch) {
        int64_t row[kHitBatch];
#pragma unroll
        for (int r = 0; r < kHitBatch; ++r) {
          const int64_t i = i0 + (int64_t)r * kBlock + threadIdx.x;
          row[r] = i < total ? tile * kHitTile + hits[i] : m;
        }
        int64_t h[kHitBatch];
        if (out_build) probe_heads<K, DIRECT, R, kHitBatch>(keys, valid, m, row, t, true, h);
#pragma unroll
        for (int r = 0; r < kHitBatch; ++r) {
          if (row[r] >= m) continue;
          const int64_t pos = base + i0 + (int64_t)r * kBlock + threadIdx.x;
          if (pos >= out_cap) continue;   // a replayed (undersized) total: see join_expand_kernel
          out_probe[pos] = (O)row[r];
          if (out_build) out_build[pos] = (R)h[r];
        }
      }
    } else if (total) {
      const int64_t base = tile_off[tile];
      // kHitBatch hit words per wave at a time (waves own words wave, wave+4, ...)
      for (int w0 = wave; w0 < nwords; w0 += kWavesPerBlock * kHitBatch) {
        unsigned long long b[kHitBatch];
        int64_t row[kHitBatch];
#pragma unroll
        for (int r = 0; r < kHitBatch; ++r) {
          const int w = w0 + r * kWavesPerBlock;
          b[r] = w < nwords ? words[tile * kHitWords + w] : 0ULL;
          // rows that are not hits are pushed past m: probe_heads skips them
          row[r] = ((b[r] >> lane) & 1ULL) ? tile * kHitTile + (int64_t)w * kWave + lane : m;
        }
        int64_t h[kHitBatch];
        if (out_build) probe_heads<K, DIRECT, R, kHitBatch>(keys, valid, m, row, t, true, h);
#pragma unroll
        for (int r = 0; r < kHitBatch; ++r) {
          if (row[r] >= m) continue;
          const int w = w0 + r * kWavesPerBlock;
          const int64_t pos = base + woff[w] + __popcll(b[r] & ((1ULL << lane) - 1ULL));
          if (pos >= out_cap) continue;   // a replayed (undersized) total: see join_expand_kernel
          out_probe[pos] = (O)row[r];
          if (out_build) out_build[pos] = (R)h[r];
        }
      }
    }
    __syncthreads();
  }
}

// probe_hits against a direct table with an exact membership bitmap (no head
// read at all: the bit decides): every lane takes 4 consecutive rows per step
// -- one 16-byte key load and one 4-byte validity load instead of 4 + 4 scalar
// loads -- and the 64-bit hit words are put together from each 16-lane group's
// nibbles. Same tiles, words and counts as probe_hits_kernel (probe_write
// reads them unchanged).
template <typename K>
__global__ __launch_bounds__(kBlock) void probe_bits_kernel(const K* __restrict__ keys,
                                                           const uint8_t* __restrict__ valid, int64_t m, BitmapView b,
                                                           bool negate, unsigned long long* __restrict__ words,
                                                           int64_t* __restrict__ tile_counts) {
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t tiles = (m + kHitTile - 1) / kHitTile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    int64_t cnt = 0;
#pragma unroll 2
    for (int g = 0; g < kBitsSteps; ++g) {
      const int64_t r0 = t * kHitTile + (int64_t)g * (kBlock * kBitsRows) + (int64_t)threadIdx.x * kBitsRows;
      K k[kBitsRows];
      uint32_t vb;
      const uint32_t in = load4_guarded(keys, valid, r0, m, k, vb);
      uint32_t nib = 0;
#pragma unroll
      for (int j = 0; j < kBitsRows; ++j) {
        const int64_t d = (int64_t)k[j] - b.kmin;
        bool ok = ((vb >> (8 * j)) & 0xffu) != 0 && d >= 0 && d < b.cap;
        if (ok) ok = (b.bits[(uint64_t)d >> 5] >> (d & 31)) & 1u;
        nib |= (ok != negate ? 1u : 0u) << j;
      }
      nib &= in;
      cnt += __popc(nib);
      const unsigned long long w = nibbles_to_word(nib, lane);
      const int64_t wrow = t * kHitTile + (int64_t)g * (kBlock * kBitsRows) + (int64_t)wave * (kWave * kBitsRows) +
                           (int64_t)(lane >> 4) * kWave;
      if ((lane & 15) == 0 && wrow < m)
        words[t * kHitWords + g * (kHitWords / kBitsSteps) + wave * kBitsRows + (lane >> 4)] = w;
    }
    store_tile_count<kWavesPerBlock>(wave_reduce_sum(cnt), tile_counts, t);
  }
}

// The same probe for large probe sides: the membership bitmap, folded
// modulo 64 KiB (word i = OR of the bitmap's words i, i + 16K, ...), sits in
// LDS; a probe key whose folded bit is clear is out without touching L2 (each
// global bitmap read moves a whole cache line for 4 useful bytes), and only
// folded hits consult the exact bitmap (none when the bitmap fits the fold:
// then the fold is exact). Workgroups of 1024 lanes, two per CU.
constexpr int kFoldWords = 16384;
constexpr int kFoldBlock = 1024;
constexpr int kFoldWaves = kFoldBlock / kWave;
constexpr int kFoldSteps = kHitTile / (kFoldBlock * kBitsRows);   // 2
constexpr int kWaveRows = kWave * kBitsRows;                      // rows of one wave's step (256)
constexpr int kWaveSteps = kHitTile / kWaveRows;                  // steps of a wave that owns a tile (32)

// The fold of a bitmap wider than kFoldWords, computed once per table
// (ops/hashing.py JoinTable keeps it): every probe workgroup copies these
// 64 KiB instead of OR-ing the whole bitmap (up to 4 MiB) again.
__global__ __launch_bounds__(kBlock) void probe_fold_build_kernel(const uint32_t* __restrict__ bits, int64_t nbw,
                                                                 uint32_t* __restrict__ fold) {
  const int i = blockIdx.x * kBlock + threadIdx.x;   // grid: kFoldWords / kBlock
  uint32_t v = 0;
#pragma unroll 8
  for (int64_t j = i; j < nbw; j += kFoldWords) v |= bits[j];
  fold[i] = v;
}

// The fold into LDS with 16-byte loads: src is the bitmap itself where it
// fits (nsrc words, zero-padded), else the pre-pass's kFoldWords words.
__device__ inline void fold_to_lds(uint32_t* fold, const uint32_t* __restrict__ src, int nsrc) {
#pragma unroll
  for (int i = threadIdx.x * 4; i < kFoldWords; i += kFoldBlock * 4) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (i + 4 <= nsrc) {
      v = *reinterpret_cast<const uint4*>(src + i);
    } else {
      if (i < nsrc) v.x = src[i];
      if (i + 1 < nsrc) v.y = src[i + 1];
      if (i + 2 < nsrc) v.z = src[i + 2];
    }
    *reinterpret_cast<uint4*>(fold + i) = v;
  }
}

// k - kmin as an unsigned value: d < cap is the whole range test. int32 keys
// whose table span lies inside int32 (NARROW: kmin >= -2^31, kmin + cap <= 2^31)
// need 32 bits only: a key below kmin wraps to at least 2^32 - (2^31 + kmin) >= cap.
template <typename K, bool NARROW> struct FoldDiff { using type = uint64_t; };
template <> struct FoldDiff<int32_t, true> { using type = uint32_t; };

// Hit bits of 4 rows (bit j: row j; rows past m are masked by the caller).
// Every lookup is unconditional (the fold index is masked into range, the
// bitmap index of a row that is already out reads word 0), so the four
// bitmap loads of a step are in flight together (see probe_heads).
template <typename K, bool NARROW>
__device__ inline uint32_t fold_test4(const K (&k)[kBitsRows], uint32_t vb, typename FoldDiff<K, NARROW>::type kmin,
                                      typename FoldDiff<K, NARROW>::type cap, const uint32_t* fold,
                                      const uint32_t* __restrict__ bits, bool exact, bool negate) {
  using D = typename FoldDiff<K, NARROW>::type;
  D d[kBitsRows];
  bool ok[kBitsRows];
#pragma unroll
  for (int j = 0; j < kBitsRows; ++j) {
    d[j] = (D)k[j] - kmin;
    const uint32_t f = fold[(uint32_t)(d[j] >> 5) & (kFoldWords - 1)] >> ((uint32_t)d[j] & 31);
    ok[j] = ((vb >> (8 * j)) & 0xffu) != 0 && d[j] < cap && (f & 1u);
  }
  if (!exact) {
    uint32_t w[kBitsRows];
#pragma unroll
    for (int j = 0; j < kBitsRows; ++j) w[j] = bits[ok[j] ? d[j] >> 5 : 0];
#pragma unroll
    for (int j = 0; j < kBitsRows; ++j) ok[j] = ok[j] && ((w[j] >> ((uint32_t)d[j] & 31)) & 1u);
  }
  uint32_t nib = 0;
#pragma unroll
  for (int j = 0; j < kBitsRows; ++j) nib |= (ok[j] != negate ? 1u : 0u) << j;
  return nib;
}

// Tile loop of the short probes (below kStreamMinRows there are fewer tiles
// than the chip has waves): all 16 waves of a workgroup share each tile.
template <typename K, bool NARROW>
__global__ __launch_bounds__(kFoldBlock) void probe_fold_kernel(const K* __restrict__ keys,
                                                               const uint8_t* __restrict__ valid, int64_t m,
                                                               BitmapView b, bool negate,
                                                               unsigned long long* __restrict__ words,
                                                               int64_t* __restrict__ tile_counts) {
  using D = typename FoldDiff<K, NARROW>::type;
  __shared__ alignas(16) uint32_t fold[kFoldWords];
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t nbw = (b.cap + 31) >> 5;
  const bool exact = nbw <= kFoldWords;
  fold_to_lds(fold, exact ? b.bits : b.fold, exact ? (int)nbw : kFoldWords);
  __syncthreads();
  const D dmin = (D)b.kmin, dcap = (D)b.cap;
  const int64_t tiles = (m + kHitTile - 1) / kHitTile;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    int64_t cnt = 0;
#pragma unroll
    for (int g = 0; g < kFoldSteps; ++g) {
      const int64_t r0 = t * kHitTile + (int64_t)g * (kFoldBlock * kBitsRows) + (int64_t)threadIdx.x * kBitsRows;
      K k[kBitsRows];
      uint32_t vb;
      const uint32_t in = load4_guarded(keys, valid, r0, m, k, vb);
      const uint32_t nib = fold_test4<K, NARROW>(k, vb, dmin, dcap, fold, b.bits, exact, negate) & in;
      cnt += __popc(nib);
      const unsigned long long w = nibbles_to_word(nib, lane);
      const int64_t wrow = t * kHitTile + (int64_t)g * (kFoldBlock * kBitsRows) +
                           (int64_t)wave * kWaveRows + (int64_t)(lane >> 4) * kWave;
      if ((lane & 15) == 0 && wrow < m)
        words[t * kHitWords + g * (kHitWords / kFoldSteps) + wave * kBitsRows + (lane >> 4)] = w;
    }
    store_tile_count<kFoldWaves>(wave_reduce_sum(cnt), tile_counts, t);
  }
}

// The long probes: every wave owns whole tiles (tile t of wave w in
// workgroup b: t = 16 b + w, then on by the number of waves launched), so
// the tile count is one wave reduction and no workgroup barrier follows the
// one behind the fold. A wave walks its tile in 32 steps of 256 rows and
// keeps the key and validity loads of the next kDepth steps in flight while
// it tests the current one -- across its tiles too: the last steps of a tile
// already load the first ones of the wave's next tile.
template <typename K> constexpr int kStreamDepth = sizeof(K) == 4 ? 4 : 2;

template <typename K, bool VALID>
__device__ inline void stream_load(const K* __restrict__ keys, const uint8_t* __restrict__ valid, int64_t r0,
                                   K (&k)[kBitsRows], uint32_t& vb) {
  load4(keys + r0, k);
  if constexpr (VALID) vb = *reinterpret_cast<const uint32_t*>(valid + r0);
  else vb = 0x01010101u;
}

template <typename K, bool NARROW, bool VALID>
__global__ __launch_bounds__(kFoldBlock, 8) void probe_stream_kernel(const K* __restrict__ keys,
                                                                 const uint8_t* __restrict__ valid, int64_t m,
                                                                 BitmapView b, bool negate,
                                                                 unsigned long long* __restrict__ words,
                                                                 int64_t* __restrict__ tile_counts) {
  using D = typename FoldDiff<K, NARROW>::type;
  constexpr int kDepth = kStreamDepth<K>;
  static_assert(kWaveSteps % kDepth == 0, "the step loop is unrolled by the depth");
  __shared__ alignas(16) uint32_t fold[kFoldWords];
  const int lane = lane_id(), wave = threadIdx.x / kWave;
  const int64_t nbw = (b.cap + 31) >> 5;
  const bool exact = nbw <= kFoldWords;
  fold_to_lds(fold, exact ? b.bits : b.fold, exact ? (int)nbw : kFoldWords);
  __syncthreads();
  const D dmin = (D)b.kmin, dcap = (D)b.cap;
  const int64_t tiles = (m + kHitTile - 1) / kHitTile;
  const int64_t full = m / kHitTile;   // tiles [0, full) have all their rows
  const int64_t stride = (int64_t)gridDim.x * kFoldWaves;
  const int64_t lrow = (int64_t)lane * kBitsRows;
  K kq[kDepth][kBitsRows];
  uint32_t vq[kDepth];
  int64_t t = (int64_t)blockIdx.x * kFoldWaves + wave;
  if (t < full) {
#pragma unroll
    for (int j = 0; j < kDepth; ++j)
      stream_load<K, VALID>(keys, valid, t * kHitTile + j * kWaveRows + lrow, kq[j], vq[j]);
  }
  for (; t < tiles; t += stride) {
    int cnt = 0;
    unsigned long long* wout = words + t * kHitWords + (lane >> 4);
    if (t < full) {
      const int64_t tn = t + stride;
      const bool nfull = tn < full;
      // the slot's refill: step s + kDepth of this tile, or of the wave's
      // next full tile; with neither left, step s's rows once more (in
      // bounds, never used)
      auto refill = [&](int j, int s) {
        int64_t pt = t;
        int ps = s + kDepth;
        if (ps >= kWaveSteps) {
          if (nfull) {
            pt = tn;
            ps -= kWaveSteps;
          } else {
            ps = s;
          }
        }
        stream_load<K, VALID>(keys, valid, pt * kHitTile + ps * kWaveRows + lrow, kq[j], vq[j]);
      };
      auto emit = [&](int s, uint32_t nib) {
        cnt += __popc(nib);
        const unsigned long long w = nibbles_to_word(nib, lane);
        if ((lane & 15) == 0) wout[s * kBitsRows] = w;
      };
      for (int s0 = 0; s0 < kWaveSteps; s0 += kDepth) {
#pragma unroll
        for (int j = 0; j < kDepth; ++j) {
          const uint32_t nib = fold_test4<K, NARROW>(kq[j], vq[j], dmin, dcap, fold, b.bits, exact, negate);
          refill(j, s0 + j);
          emit(s0 + j, nib);
        }
      }
    } else {
      // the probe's last tile, partly filled: guarded loads, no pipeline
      for (int s = 0; s < kWaveSteps; ++s) {
        const int64_t r0 = t * kHitTile + s * kWaveRows + lrow;
        K k[kBitsRows];
        uint32_t vb;
        const uint32_t in = load4_guarded(keys, valid, r0, m, k, vb);
        const uint32_t nib = fold_test4<K, NARROW>(k, vb, dmin, dcap, fold, b.bits, exact, negate) & in;
        cnt += __popc(nib);
        const unsigned long long w = nibbles_to_word(nib, lane);
        if ((lane & 15) == 0 && t * kHitTile + s * kWaveRows + (int64_t)(lane >> 4) * kWave < m)
          wout[s * kBitsRows] = w;
      }
    }
    const int64_t total = wave_reduce_sum((int64_t)cnt);
    if (lane == 0) tile_counts[t] = total;
  }
}

// ---- GROUP BY ----------------------------------------------------------------
// First-row table of a GROUP BY. Hashed keys (!DIRECT) go through a small
// per-workgroup LDS cache of (slot -> smallest row): rows of a hot group take
// an LDS atomic, and each workgroup sends one global atomicMin per cached slot
// at the end. Without it a low-cardinality GROUP BY (Q22's 7 country codes
// over 636K rows) had every wave's atomics -- and reads -- queue on the same
// few L2 lines: 262 us for 636K rows. Slots the cache cannot hold (a
// high-cardinality GROUP BY) take the global path directly.
constexpr int kRowCache = 256;

template <typename K, bool DIRECT>
__global__ __launch_bounds__(kBlock) void groupby_build_kernel(const K* __restrict__ keys, int64_t n,
                                                              int64_t* __restrict__ tkeys, int32_t* __restrict__ trow,
                                                              int64_t cap, int64_t kmin) {
  __shared__ int32_t cslot[DIRECT ? 1 : kRowCache];
  __shared__ int32_t crow[DIRECT ? 1 : kRowCache];
  if (!DIRECT) {
    for (int h = threadIdx.x; h < kRowCache; h += blockDim.x) {
      cslot[h] = -1;
      crow[h] = INT32_MAX;
    }
    __syncthreads();
  }
  const int64_t mask = cap - 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t k = (int64_t)keys[i];
    int64_t slot;
    if (DIRECT) {
      slot = k - kmin;
      // a key outside the span only occurs under a replayed key range that the
      // end-of-query check will reject (ops/_lib.py Speculation): stay in bounds
      if ((uint64_t)slot >= (uint64_t)cap) continue;
    } else {
      bool existed;
      slot = insert_slot(tkeys, mask, k, &existed);
      const int h = (int)(slot & (kRowCache - 1));
      int cur = cap < ((int64_t)1 << 31) ? cslot[h] : -2;    // (slots, the reserved one included, must fit the int32 cache)
      if (cur == -1) {
        cur = atomicCAS(&cslot[h], -1, (int32_t)slot);
        if (cur == -1) cur = (int32_t)slot;
      }
      if (cur == (int32_t)slot) {
        atomicMin(&crow[h], (int32_t)i);
        continue;
      }
    }
    // first occurrence row: plain read first avoids most atomics on hot groups
    if (trow[slot] > (int32_t)i) atomicMin(&trow[slot], (int32_t)i);
  }
  if (!DIRECT) {
    __syncthreads();
    for (int h = threadIdx.x; h < kRowCache; h += blockDim.x)
      if (cslot[h] >= 0 && trow[cslot[h]] > crow[h]) atomicMin(&trow[cslot[h]], crow[h]);
  }
}

// Direct-mapped GROUP BY over a small key span (Q5's 5 nations, Q7/Q9's
// (nation, year) pairs over millions of rows): the first-row table lives in
// LDS per workgroup, so the atomics that would serialise on a handful of
// global words stay on-chip; one global atomicMin per touched slot per
// workgroup at the end.
constexpr int64_t kGroupLdsSlots = 16384;

template <typename K>
__global__ __launch_bounds__(kBlock) void groupby_build_lds_kernel(const K* __restrict__ keys, int64_t n,
                                                                  int32_t* __restrict__ trow, int64_t cap,
                                                                  int64_t kmin) {
  __shared__ int32_t srow[kGroupLdsSlots];
  for (int64_t s = threadIdx.x; s < cap; s += blockDim.x) srow[s] = INT32_MAX;
  __syncthreads();
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t slot = (int64_t)keys[i] - kmin;
    if ((uint64_t)slot >= (uint64_t)cap) continue;   // see groupby_build_kernel
    if (srow[slot] > (int32_t)i) atomicMin(&srow[slot], (int32_t)i);
  }
  __syncthreads();
  for (int64_t s = threadIdx.x; s < cap; s += blockDim.x) {
    const int32_t r = srow[s];
    if (r != INT32_MAX && trow[s] > r) atomicMin(&trow[s], r);
  }
}

// also zeroes gid_of_slot: a slot the (replayed) group count leaves unassigned
// then maps to group 0 instead of an uninitialised id (see groupby_build_kernel)
__global__ __launch_bounds__(kBlock) void occupied_kernel(const int32_t* __restrict__ trow, int64_t cap,
                                                         uint8_t* __restrict__ occ, int32_t* __restrict__ gid_of_slot) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cap; i += (int64_t)gridDim.x * blockDim.x) {
    occ[i] = trow[i] != INT32_MAX;
    gid_of_slot[i] = 0;
  }
}

// gid_of_slot[slots[g]] = g ; rep_row[g] = trow[slots[g]]
template <typename S>
__global__ __launch_bounds__(kBlock) void assign_gid_kernel(const S* __restrict__ slots, int64_t g, int64_t cap,
                                                           const int32_t* __restrict__ trow,
                                                           int32_t* __restrict__ gid_of_slot,
                                                           int32_t* __restrict__ rep_row) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < g; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t s = (int64_t)slots[i];
    if ((uint64_t)s >= (uint64_t)cap) {   // a replayed group count past the real one: unwritten slot ids
      rep_row[i] = 0;
      continue;
    }
    gid_of_slot[s] = (int32_t)i;
    rep_row[i] = trow[s];
  }
}

template <typename K, bool DIRECT>
__global__ __launch_bounds__(kBlock) void groupby_lookup_kernel(const K* __restrict__ keys, int64_t n,
                                                               const int64_t* __restrict__ tkeys,
                                                               const int32_t* __restrict__ gid_of_slot, int64_t cap,
                                                               int64_t kmin, int32_t* __restrict__ gid) {
  const int64_t mask = cap - 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t k = (int64_t)keys[i];
    int64_t slot = DIRECT ? k - kmin : find_slot(tkeys, mask, k);
    if (DIRECT && (uint64_t)slot >= (uint64_t)cap) slot = 0;   // see groupby_build_kernel
    gid[i] = gid_of_slot[slot];
  }
}

template <typename I>
__global__ __launch_bounds__(kBlock) void fill_runs_kernel(const I* __restrict__ starts, int64_t nruns, int64_t n,
                                                          int32_t* __restrict__ gid) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nruns; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t b = starts[r], e = r + 1 < nruns ? (int64_t)starts[r + 1] : n;
    // a replayed run count can leave the starts' tail unwritten: stay in [0, n)
    b = b < 0 ? 0 : (b > n ? n : b);
    e = e < b ? b : (e > n ? n : e);
    for (int64_t i = b; i < e; ++i) gid[i] = (int32_t)r;
  }
}

[[noreturn]] void null_buffer(const char* what) { throw std::runtime_error(std::string(what) + ": null buffer"); }

}  // namespace

// ---- host entry points -------------------------------------------------------
void check(const JoinTableRef& t, const char* what) {
  if (!t.thead || (!t.direct && !t.tkeys) || (!t.cstart != !t.crows)) null_buffer(what);
}

void join_table_init(void* thead, bool rid64, int64_t cap, int64_t* tkeys, uint32_t* bits, int64_t nbw,
                     unsigned long long* dups, hipStream_t stream) {
  if ((((uintptr_t)thead | (uintptr_t)tkeys | (uintptr_t)bits) & 15) || ((uintptr_t)dups & 7))
    throw std::runtime_error("join_table_init: buffers must be 16-byte aligned");
  const FillSeg a{static_cast<uint32_t*>(thead), rid64 ? 2 * cap : cap, 0xffffffffu, 0xffffffffu};
  const FillSeg k{reinterpret_cast<uint32_t*>(tkeys), tkeys ? 2 * cap : 0, (uint32_t)(uint64_t)kEmptyKey,
                  (uint32_t)((uint64_t)kEmptyKey >> 32)};
  const FillSeg z{bits, bits ? nbw : 0, 0u, 0u};
  const int64_t chunks = (a.words >> 2) + (k.words >> 2) + (z.words >> 2);
  launch("join_table_init", join_table_init_kernel, dim3(grid_for(chunks, kBlock, 2048)), dim3(kBlock), 0, stream, a, k,
         z, dups);
}

void join_build(const JoinTableRef& t, const KeyColumn& c, unsigned long long* dups, hipStream_t stream) {
  if (c.n == 0) return;
  check(t, "join_build");
  if (!c.keys || !dups) null_buffer("join_build");
  dim3 g(grid_for(c.n, kBlock, kMaxGrid)), b(kBlock);
  dispatch(wide{c.key64}, t.direct, wide{t.rid64}, [&](auto k, auto d, auto r) {
    using K = type_of<decltype(k)>;
    using R = type_of<decltype(r)>;
    launch("join_build", join_build_kernel<K, d.value, R>, g, b, 0, stream, as<K>(c.keys), c.valid, c.n,
           view<R, true>(t), dups);
  });
}

void join_csr_count(const JoinTableRef& t, const KeyColumn& c, void* cnt, hipStream_t stream) {
  if (c.n == 0) return;
  check(t, "join_csr_count");
  if (!c.keys || !cnt) null_buffer("join_csr_count");
  dim3 g(grid_for(c.n, kBlock, kMaxGrid)), b(kBlock);
  dispatch(wide{c.key64}, t.direct, wide{t.rid64}, [&](auto k, auto d, auto r) {
    using K = type_of<decltype(k)>;
    using R = type_of<decltype(r)>;
    launch("join_csr_count", join_csr_count_kernel<K, d.value, R>, g, b, 0, stream, as<K>(c.keys), c.valid, c.n,
           view<R>(t), as<R>(cnt));
  });
}

void join_csr_scatter(const JoinTableRef& t, const KeyColumn& c, void* cnt, hipStream_t stream) {
  if (c.n == 0) return;
  check(t, "join_csr_scatter");
  if (!c.keys || !cnt || !t.cstart) null_buffer("join_csr_scatter");
  dim3 g(grid_for(c.n, kBlock, kMaxGrid)), b(kBlock);
  dispatch(wide{c.key64}, t.direct, wide{t.rid64}, [&](auto k, auto d, auto r) {
    using K = type_of<decltype(k)>;
    using R = type_of<decltype(r)>;
    launch("join_csr_scatter", join_csr_scatter_kernel<K, d.value, R>, g, b, 0, stream, as<K>(c.keys), c.valid, c.n,
           view<R>(t), as<R>(cnt), as<R>(t.crows));
  });
}

void join_probe(const JoinTableRef& t, const KeyColumn& c, bool use_filter, int32_t* counts, void* first,
                uint8_t* build_matched, hipStream_t stream) {
  const int64_t m = c.n;
  if (m == 0) return;
  check(t, "join_probe");
  if (!c.keys) null_buffer("join_probe");
  const dim3 b(kBlock);
  const bool first_direct = t.direct && first && !counts && !build_matched && !t.cstart;
  dispatch(wide{c.key64}, t.direct, wide{t.rid64}, [&](auto k, auto d, auto r) {
    using K = type_of<decltype(k)>;
    using R = type_of<decltype(r)>;
    if constexpr (d.value) {
      if (first_direct) {
        const dim3 g4(grid_for((m + kProbeRows - 1) / kProbeRows, kBlock, kMaxGrid));
        launch("join_probe_first_direct", join_probe_first_direct_kernel<K, R>, g4, b, 0, stream, as<K>(c.keys),
               c.valid, m, view<R>(t, use_filter), as<R>(first));
        return;
      }
    }
    const dim3 g(grid_for(m, kBlock, kMaxGrid));
    launch("join_probe", join_probe_kernel<K, d.value, R>, g, b, 0, stream, as<K>(c.keys), c.valid, m,
           view<R>(t, use_filter), counts, as<R>(first), build_matched);
  });
}

void join_expand(const JoinTableRef& t, const KeyColumn& c, bool use_filter, const int64_t* offsets,
                 int32_t* out_probe, void* out_build, int64_t out_cap, hipStream_t stream) {
  if (c.n == 0) return;
  check(t, "join_expand");
  if (!c.keys || !offsets || !out_probe || !out_build) null_buffer("join_expand");
  dim3 g(grid_for(c.n, kBlock, kMaxGrid)), b(kBlock);
  dispatch(wide{c.key64}, t.direct, wide{t.rid64}, [&](auto k, auto d, auto r) {
    using K = type_of<decltype(k)>;
    using R = type_of<decltype(r)>;
    launch("join_expand", join_expand_kernel<K, d.value, R>, g, b, 0, stream, as<K>(c.keys), c.valid, c.n,
           view<R>(t, use_filter), offsets, out_probe, as<R>(out_build), out_cap);
  });
}

int64_t probe_hit_tiles(int64_t m) { return (m + kHitTile - 1) / kHitTile; }

// workgroups of a probe_hits / probe_write launch at most (both loop over
// their tiles): tunable for the A/B in scripts/bench_probe.py
static int g_probe_grid_cap = 1 << 16;
void set_probe_grid_cap(int cap) { g_probe_grid_cap = cap > 0 ? cap : (1 << 16); }
// 0: scalar probe_hits_kernel only, 1: + the vector bitmap probe, 2: + the LDS-folded
// bitmap for large probe sides (scripts/bench_probe.py A/B)
static int g_probe_bits = 2;
void set_probe_bits(int mode) { g_probe_bits = mode; }
constexpr int64_t kFoldMinRows = 1 << 22;   // below: copying the fold per workgroup does not pay
constexpr int64_t kFoldGrid = 512;          // two 1024-lane workgroups (64 KiB LDS each) per CU
int64_t probe_fold_min_rows() { return kFoldMinRows; }
int probe_fold_words() { return kFoldWords; }

// probe_stream_kernel takes the probes of which every wave of its grid owns
// a tile or more (512 workgroups x 16 waves x 8192 rows = 64M rows) -- below,
// the tile loop of probe_fold_kernel keeps the chip filled -- and whose fold
// filters well. A bitmap wider than the fold ORs nbw / 16384 words into each
// folded bit: with n build keys over cap slots about
// 1 - (1 - n/cap)^(nbw/16384) of the folded bits are set, and every key that
// passes the fold costs a bitmap read from L2 that the streaming loop hides
// worse than the tile loop does. probe_hits alone on an MI355X, int32 keys,
// half the rows masked, tile loop / streaming loop in ms:
//   fill 0.07 (40K keys over 1M): 0.043 / 0.043 at 32M rows, 0.093 / 0.083
//     at 64M, 0.768 / 0.705 at 600M (TPC-H Q21's probe)
//   exact fold (40K over 500K):   0.079 / 0.072 at 64M, 0.646 / 0.622 at 600M
//   fill 0.11: 0.769 / 0.751 at 600M    fill 0.15: 0.778 / 0.793
//   fill 0.25: 0.832 / 0.941            fill 0.88 (1.1M over 20M): 1.526 / 1.818
// probe_bits_kernel took 1.466 ms at fill 0.07 and 1.780 ms at fill 0.88 (600M
// rows): behind the tile loop at every fill, so no fill hands a probe to it.
constexpr int64_t kStreamMinRows = kFoldGrid * kFoldWaves * kHitTile;
constexpr double kStreamMaxFill = 0.1;
static int64_t g_stream_min_rows = kStreamMinRows;
static double g_stream_max_fill = kStreamMaxFill;
void set_probe_stream_min_rows(int64_t rows) { g_stream_min_rows = rows >= 0 ? rows : kStreamMinRows; }
void set_probe_stream_max_fill(double fill) { g_stream_max_fill = fill >= 0 ? fill : kStreamMaxFill; }

enum ProbeKernel { kProbeNone = 0, kProbeScalar, kProbeBits, kProbeFold, kProbeStream };
static ProbeKernel g_last_probe = kProbeNone;
const char* last_probe_kernel() {
  static const char* const names[] = {"none", "hits", "bits", "fold", "stream"};
  return names[g_last_probe];
}

// which kernel serves a probe of m rows; vec: a direct table with an exact
// bitmap and buffers aligned for the vector loads
static ProbeKernel probe_plan(bool vec, int64_t m, int64_t cap, int64_t n_build) {
  if (!vec || g_probe_bits < 1) return kProbeScalar;
  if (g_probe_bits < 2 || m < kFoldMinRows) return kProbeBits;
  if (m < g_stream_min_rows) return kProbeFold;
  const int64_t nbw = (cap + 31) >> 5;
  if (nbw > kFoldWords) {
    const double load = n_build < cap ? (double)n_build / (double)cap : 1.0;
    if (1.0 - std::pow(1.0 - load, (double)nbw / kFoldWords) > g_stream_max_fill) return kProbeFold;
  }
  return kProbeStream;
}

bool probe_fold_needed(int64_t m, int64_t cap) {
  return ((cap + 31) >> 5) > kFoldWords && probe_plan(true, m, cap, 0) >= kProbeFold;
}

void probe_fold_build(const uint32_t* bits, int64_t cap, uint32_t* fold, hipStream_t stream) {
  launch("probe_fold_build", probe_fold_build_kernel, dim3(kFoldWords / kBlock), dim3(kBlock), 0, stream, bits,
         (cap + 31) >> 5, fold);
}

void probe_hits(const JoinTableRef& t, const KeyColumn& c, bool use_filter, bool negate, unsigned long long* words,
                int64_t* tile_counts, hipStream_t stream) {
  const int64_t m = c.n;
  if (m == 0) return;
  check(t, "probe_hits");
  if (!c.keys || !words || !tile_counts) null_buffer("probe_hits");
  const BitmapView bm{use_filter ? t.bits : nullptr, t.fold, t.cap, t.kmin};
  const dim3 g(grid_for(probe_hit_tiles(m), 1, g_probe_grid_cap)), b(kBlock);
  const bool vec = t.direct && bm.bits && (t.bmask & kExactBits) && ((uintptr_t)c.keys & 15) == 0 &&
                   ((uintptr_t)c.valid & 3) == 0;
  ProbeKernel plan = probe_plan(vec, m, t.cap, t.n_build);
  // (the fold kernels copy the bitmap, or its fold, with 16-byte loads)
  if (plan >= kProbeFold && (((uintptr_t)bm.bits | (uintptr_t)bm.fold) & 15)) plan = kProbeBits;
  g_last_probe = plan;
  if (plan >= kProbeFold) {
    if (((t.cap + 31) >> 5) > kFoldWords && !bm.fold)
      throw std::runtime_error("probe_hits: a bitmap wider than the fold needs probe_fold_build's scratch");
    const bool narrow = !c.key64 && t.kmin >= INT32_MIN && t.cap < (1LL << 31) && t.kmin + t.cap <= (1LL << 31);
    const int64_t tiles = probe_hit_tiles(m);
    const dim3 bf(kFoldBlock);
    dispatch(wide{c.key64}, narrow, c.valid != nullptr, [&](auto k, auto nr, auto v) {
      using K = type_of<decltype(k)>;
      if constexpr (sizeof(K) == 4 || !nr.value) {  // NARROW exists for int32 keys only
        if (plan == kProbeFold)
          launch("probe_hits", probe_fold_kernel<K, nr.value>, dim3(grid_for(tiles, 1, kFoldGrid)), bf, 0, stream,
                 as<K>(c.keys), c.valid, m, bm, negate, words, tile_counts);
        else
          launch("probe_hits", probe_stream_kernel<K, nr.value, v.value>, dim3(grid_for(tiles, kFoldWaves, kFoldGrid)),
                 bf, 0, stream, as<K>(c.keys), c.valid, m, bm, negate, words, tile_counts);
      }
    });
  } else if (plan == kProbeBits) {
    dispatch(wide{c.key64}, [&](auto k) {
      using K = type_of<decltype(k)>;
      launch("probe_hits", probe_bits_kernel<K>, g, b, 0, stream, as<K>(c.keys), c.valid, m, bm, negate, words,
             tile_counts);
    });
  } else {
    dispatch(wide{c.key64}, t.direct, wide{t.rid64}, [&](auto k, auto d, auto r) {
      using K = type_of<decltype(k)>;
      using R = type_of<decltype(r)>;
      launch("probe_hits", probe_hits_kernel<K, d.value, R>, g, b, 0, stream, as<K>(c.keys), c.valid, m,
             view<R>(t, use_filter), negate, words, tile_counts);
    });
  }
}

void probe_write(const JoinTableRef& t, const KeyColumn& c, const unsigned long long* words, const int64_t* tile_off,
                 void* out_probe, bool out64, void* out_build, int64_t out_cap, hipStream_t stream) {
  if (c.n == 0) return;
  check(t, "probe_write");
  if (!c.keys || !words || !tile_off || !out_probe) null_buffer("probe_write");
  const dim3 g(grid_for(probe_hit_tiles(c.n), 1, g_probe_grid_cap)), b(kBlock);
  dispatch(wide{c.key64}, t.direct, wide{t.rid64}, wide{out64}, [&](auto k, auto d, auto r, auto o) {
    using K = type_of<decltype(k)>;
    using R = type_of<decltype(r)>;
    using O = type_of<decltype(o)>;
    launch("probe_write", probe_write_kernel<K, d.value, R, O>, g, b, 0, stream, as<K>(c.keys), c.valid, c.n,
           view<R>(t), words, tile_off, as<O>(out_probe), as<R>(out_build), out_cap);
  });
}

void fill_runs(const void* starts, bool starts64, int64_t nruns, int64_t n, int32_t* gid, hipStream_t stream) {
  if (nruns == 0) return;
  dim3 g(grid_for(nruns, kBlock, kMaxGrid)), b(kBlock);
  dispatch(wide{starts64}, [&](auto i) {
    using I = type_of<decltype(i)>;
    launch("fill_runs", fill_runs_kernel<I>, g, b, 0, stream, as<I>(starts), nruns, n, gid);
  });
}

void groupby_build(const void* keys, bool key64, int64_t n, int64_t* tkeys, int32_t* trow, int64_t cap, int64_t kmin,
                   bool direct, hipStream_t stream) {
  if (n == 0) return;
  const bool lds = direct && cap <= kGroupLdsSlots;
  dispatch(wide{key64}, direct, [&](auto k, auto d) {
    using K = type_of<decltype(k)>;
    const dim3 b(kBlock);
    if (lds) {
      // a few hundred workgroups: enough to fill the CUs, few end-of-block merges
      const dim3 g(grid_for(n, kBlock * 16, 1024));
      launch("groupby_build_lds", groupby_build_lds_kernel<K>, g, b, 0, stream, as<K>(keys), n, trow, cap, kmin);
      return;
    }
    // (hashed: several rows per lane, so each workgroup's row cache covers many rows)
    const dim3 g(grid_for(n, direct ? kBlock : kBlock * 8, kMaxGrid));
    launch("groupby_build", groupby_build_kernel<K, d.value>, g, b, 0, stream, as<K>(keys), n, tkeys, trow, cap, kmin);
  });
}

void groupby_occupied(const int32_t* trow, int64_t cap, uint8_t* occ, int32_t* gid_of_slot, hipStream_t stream) {
  launch("groupby_occupied", occupied_kernel, dim3(grid_for(cap, kBlock, kMaxGrid)), dim3(kBlock), 0, stream, trow, cap,
         occ, gid_of_slot);
}

void groupby_assign(const void* slots, bool slots64, int64_t g, int64_t cap, const int32_t* trow,
                    int32_t* gid_of_slot, int32_t* rep_row, hipStream_t stream) {
  if (g == 0) return;
  dim3 gr(grid_for(g, kBlock, kMaxGrid)), b(kBlock);
  dispatch(wide{slots64}, [&](auto s) {
    using S = type_of<decltype(s)>;
    launch("groupby_assign", assign_gid_kernel<S>, gr, b, 0, stream, as<S>(slots), g, cap, trow, gid_of_slot, rep_row);
  });
}

void groupby_lookup(const void* keys, bool key64, int64_t n, const int64_t* tkeys, const int32_t* gid_of_slot,
                    int64_t cap, int64_t kmin, bool direct, int32_t* gid, hipStream_t stream) {
  if (n == 0) return;
  dim3 g(grid_for(n, kBlock, kMaxGrid)), b(kBlock);
  dispatch(wide{key64}, direct, [&](auto k, auto d) {
    using K = type_of<decltype(k)>;
    launch("groupby_lookup", groupby_lookup_kernel<K, d.value>, g, b, 0, stream, as<K>(keys), n, tkeys, gid_of_slot,
           cap, kmin, gid);
  });
}

}  // namespace kern
}  // namespace igloo
