// UTF-8 string kernels over Arrow large-string layout (int64 offsets + bytes).
//
// * str_like: SQL LIKE/ILIKE with '%' and '_' (pattern pre-tokenised on the
//   host so escapes are already resolved). Greedy wildcard matching with a
//   single backtrack point: linear in the usual case.
// * str_case: upper/lower — the reference's `capitalize` UDF uppercases the
//   whole string (reference crates/engine/src/lib.rs:84-91). ASCII bytes are
//   mapped on the GPU; the kernel reports whether any non-ASCII byte was seen
//   so the host can fall back to full Unicode case mapping.
// * str_substr: SUBSTRING(s FROM a FOR b) in characters (UTF-8 aware).
// * str_hash64 / str_eq_rows / str_cmp_const: hashing and comparisons for
//   GROUP BY, join verification and predicates on plain string columns.
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace igloo {
namespace kern {

namespace {

__device__ inline uint8_t fold(uint8_t c, bool ci) { return ci && c >= 'A' && c <= 'Z' ? c + 32 : c; }

__device__ bool like_match(const uint8_t* s, int64_t n, const uint8_t* pat, const uint8_t* kind, int m, bool ci) {
  int64_t si = 0, ss = 0;
  int pi = 0, star = -1;
  while (si < n) {
    if (pi < m && (kind[pi] == 1 || (kind[pi] == 0 && fold(pat[pi], ci) == fold(s[si], ci)))) {
      // '_' consumes one UTF-8 character
      if (kind[pi] == 1) {
        ++si;
        while (si < n && (s[si] & 0xC0) == 0x80) ++si;
      } else {
        ++si;
      }
      ++pi;
    } else if (pi < m && kind[pi] == 2) {
      star = pi++;
      ss = si;
    } else if (star != -1) {
      pi = star + 1;
      si = ++ss;
    } else {
      return false;
    }
  }
  while (pi < m && kind[pi] == 2) ++pi;
  return pi == m;
}

__global__ __launch_bounds__(kBlock) void like_kernel(const int64_t* __restrict__ off, const uint8_t* __restrict__ chars,
                                                     int64_t n, const uint8_t* __restrict__ pat,
                                                     const uint8_t* __restrict__ kind, int m, bool ci, bool negate,
                                                     uint8_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = off[i];
    bool r = like_match(chars + a, off[i + 1] - a, pat, kind, m, ci);
    out[i] = r != negate;
  }
}

// LDS-staged LIKE: a block takes 256 consecutive strings, copies their byte
// range into LDS with 16-byte coalesced loads, then each lane matches its
// string out of LDS. The per-lane byte-serial scan of the simple kernel above
// touches a new 64-byte line every few bytes per lane; staging turns the HBM
// traffic into one streaming read of the character buffer.
constexpr int kLikeTileBytes = 16384;  // 256 rows of ~50-byte comments; 24.6 KB LDS per block -> 6 blocks per CU
constexpr int kLikeMaxPattern = 256;

__global__ __launch_bounds__(kBlock) void like_tile_kernel(const int64_t* __restrict__ off,
                                                          const uint8_t* __restrict__ chars, int64_t n,
                                                          const uint8_t* __restrict__ pat,
                                                          const uint8_t* __restrict__ kind, int m, bool ci,
                                                          bool negate, uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[kLikeTileBytes];
  __shared__ uint8_t spat[kLikeMaxPattern], skind[kLikeMaxPattern];
  for (int i = threadIdx.x; i < m; i += kBlock) {
    spat[i] = pat[i];
    skind[i] = kind[i];
  }
  const int64_t tiles = (n + kBlock - 1) / kBlock;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i0 = t * kBlock;
    const int64_t i1 = i0 + kBlock < n ? i0 + kBlock : n;
    const uintptr_t lo = (uintptr_t)(chars + off[i0]);
    const uintptr_t hi = (uintptr_t)(chars + off[i1]);
    const uintptr_t start = lo & ~(uintptr_t)15;       // never below the allocation (>= 256 B aligned)
    const uintptr_t full_end = hi & ~(uintptr_t)15;    // vector loads stop here; the tail goes bytewise
    const bool staged = hi - start <= (uintptr_t)kLikeTileBytes;
    __syncthreads();  // previous tile finished reading buf; pattern visible on the first pass
    if (staged) {
      const int64_t nvec = (int64_t)(full_end - start) / 16;
      for (int64_t v = threadIdx.x; v < nvec; v += kBlock)
        *(uint4*)(buf + v * 16) = *(const uint4*)(start + v * 16);
      for (uintptr_t a = full_end + threadIdx.x; a < hi; a += kBlock) buf[a - start] = *(const uint8_t*)a;
    }
    __syncthreads();
    const int64_t i = i0 + threadIdx.x;
    if (i < i1) {
      const int64_t a = off[i], len = off[i + 1] - a;
      bool r;
      if (staged)
        r = like_match(buf + ((uintptr_t)(chars + a) - start), len, spat, skind, m, ci);
      else
        r = like_match(chars + a, len, spat, skind, m, ci);
      out[i] = r != negate;
    }
  }
}

// LIKE over '%'-separated literal segments (no '_', case-sensitive) — the
// shape of nearly every analytic LIKE: 'PROMO%', '%BRASS', '%green%',
// '%special%requests%'. Two kernels (str_like_segments routes):
//   * like_stream_kernel, further down: 1-2 segments of >= 7 bytes each. The
//     column is scanned as one byte stream and rows are looked at only where
//     an aligned dword of the longest segment shows up;
//   * like_seg_kernel, here: everything else (short segments, 3-4 segments).
// like_seg_kernel, per tile of 256 strings staged in LDS:
//   1. every lane takes 16-byte chunks of the tile and marks, for every
//      segment, the positions where it starts: 4-byte windows built with
//      v_alignbyte from five dwords are compared against the segment prefix in
//      registers, the rare candidates are verified byte-wise, and the 16-bit
//      mask goes to an LDS bitmap (one LDS read per 16 positions);
//   2. each lane then walks its string greedily: the earliest hit of segment 0
//      at/after the cursor, then segment 1 after that, ... using bit scans.
// (A variant that prefetches the next tile into registers while matching the
// current one, with the chunk tail taken by a lane shuffle, measured 6.2 ms
// against this kernel's 5.0 ms for Q13 at SF100: the extra registers cost
// more occupancy than the overlap gained. Removing the LDS bank conflicts --
// the window's fifth dword from the neighbouring lane, mask pairs stored as
// one dword -- took them from 54M to 0.2M per suite but ran 3 % slower:
// profiles/r4_select_like_ab.txt.)
constexpr int kSegMax = 4;

__device__ inline int next_hit(const uint64_t* bits, int from, int last) {
  // smallest p in [from, last] with bit p set, or -1
  if (from > last) return -1;
  int w = from >> 6;
  uint64_t word = bits[w] & (~0ULL << (from & 63));
  const int lw = last >> 6;
  while (true) {
    if (word) {
      const int p = (w << 6) + __builtin_ctzll(word);
      return p <= last ? p : -1;
    }
    if (++w > lw) return -1;
    word = bits[w];
  }
}

// Greedy walk of one row [b0, b1) of a tile over the per-segment hit bitmaps:
// the earliest hit of segment 0 at/after the cursor, then segment 1 after it, ...
template <int SEGS, int WORDS>
__device__ inline bool seg_walk(const uint64_t (&bits)[SEGS][WORDS], const int32_t* soff, int nseg, bool anchor_start,
                                bool anchor_end, int b0, int b1) {
  int cur = b0;
  bool r = true;
  for (int sg = 0; sg < nseg && r; ++sg) {
    const int sl = soff[sg + 1] - soff[sg];
    const bool last = sg == nseg - 1;
    if (sg == 0 && anchor_start) {
      r = cur + sl <= b1 && ((bits[0][cur >> 6] >> (cur & 63)) & 1ULL);
      cur += sl;
    } else if (last && anchor_end) {
      const int p = b1 - sl;
      r = p >= cur && ((bits[sg][p >> 6] >> (p & 63)) & 1ULL);
      cur = b1;
    } else {
      const int p = next_hit(bits[sg], cur, b1 - sl);
      r = p >= 0;
      cur = p + sl;
    }
  }
  if (r && anchor_end && (nseg == 0 || (nseg == 1 && anchor_start))) r = cur == b1;
  return r;
}

// unaligned loads (global memory takes any alignment; one instruction each)
__device__ inline uint32_t load_u32(const uint8_t* p) {
  uint32_t x;
  __builtin_memcpy(&x, p, 4);
  return x;
}
__device__ inline uint4 load_u128(const uint8_t* p) {
  uint4 x;
  __builtin_memcpy(&x, p, 16);
  return x;
}

// The exact matcher on one string s[0, L) in global memory, literal by
// literal: the leftmost occurrence of each segment after the previous one.
// Never reads outside the string.
// kDword = false: byte by byte, any segment length. Every byte is a load
// that depends on the one before, so this is for the rare oversized tile.
// kDword = true, every segment >= 7 bytes: a few rounds of independent loads
// per string. An occurrence at p contains, for any 4-byte grid, the grid's
// dword at p rounded up, which equals the segment's bytes at 0..3 + (0..3);
// so 16-byte pieces of the string (four at a time, the last one read
// overlapping so that it ends at L) are tested dword by dword against those
// four windows and only a hit is compared in full, with dword loads.
template <bool kDword>
__device__ inline bool seg_search(const uint8_t* s, int64_t L, const uint8_t* sseg, const int32_t* soff, int nseg,
                                  bool anchor_start, bool anchor_end) {
  int64_t cur = 0;
  bool r = true;
  for (int sg = 0; sg < nseg && r; ++sg) {
    const int s0 = soff[sg], sl = soff[sg + 1] - s0;
    const bool last = sg == nseg - 1;
    auto seg_u32 = [&](int k) {
      return (uint32_t)sseg[s0 + k] | ((uint32_t)sseg[s0 + k + 1] << 8) | ((uint32_t)sseg[s0 + k + 2] << 16) |
             ((uint32_t)sseg[s0 + k + 3] << 24);
    };
    auto eq = [&](int64_t p) {   // p + sl <= L
      if constexpr (kDword) {
        // dwords at 0, 4, 8, 12 (the last one moved back to end at sl): loads that do not wait for each other
        uint32_t diff = 0;
#pragma unroll
        for (int k = 0; k < 16; k += 4) {
          const int o = k < sl - 4 ? k : sl - 4;
          diff |= load_u32(s + p + o) ^ seg_u32(o);
        }
        for (int k = 16; k < sl && !diff; k += 4) {
          const int o = k < sl - 4 ? k : sl - 4;
          diff |= load_u32(s + p + o) ^ seg_u32(o);
        }
        return diff == 0;
      } else {
        for (int k = 0; k < sl; ++k)
          if (s[p + k] != sseg[s0 + k]) return false;
        return true;
      }
    };
    // smallest p >= from with p + sl <= L where the segment occurs, or -1
    auto find = [&](int64_t from) -> int64_t {
      if constexpr (kDword) {
        if (from + sl > L) return -1;
        const uint32_t W[4] = {seg_u32(0), seg_u32(1), seg_u32(2), seg_u32(3)};
        // the piece at string position c: occurrences whose grid dword it holds, in ascending order
        auto scan = [&](const uint4& v, int64_t c) -> int64_t {
          uint32_t m = ~0u;
#pragma unroll
          for (int o = 0; o < 4; ++o) m = min(min(m, v.x ^ W[o]), min(min(v.y ^ W[o], v.z ^ W[o]), v.w ^ W[o]));
          if (m) return -1;
          const uint32_t d[4] = {v.x, v.y, v.z, v.w};
          uint32_t hits = 0;   // bit 4 w + 3 - o: dword w equals window o, i.e. a start at c + 4 w - o
#pragma unroll
          for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int o = 0; o < 4; ++o) hits |= (uint32_t)(d[w] == W[o]) << (4 * w + 3 - o);
          for (; hits; hits &= hits - 1) {
            const int64_t p = c + __builtin_ctz(hits) - 3;   // ascending
            if (p >= from && p + sl <= L && eq(p)) return p;
          }
          return -1;
        };
        if (L < 16) {   // one zero-filled piece holds the string
          uint32_t d[4] = {0, 0, 0, 0};
          for (int k = 0; k < (int)L; ++k) d[k >> 2] |= (uint32_t)s[k] << (8 * (k & 3));
          return scan(uint4{d[0], d[1], d[2], d[3]}, 0);
        }
        // pieces on the grid of the string's start; one that would pass the
        // end is read at L - 16 instead: on its own grid it still holds a
        // dword of every occurrence not seen in the pieces before it
        for (int64_t c = from & ~(int64_t)15; c < L; c += 64) {
          int64_t cc[4];
          uint4 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            cc[u] = c + 16 * u < L - 16 ? c + 16 * u : L - 16;
            v[u] = load_u128(s + cc[u]);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (u && c + 16 * u >= L) break;
            const int64_t p = scan(v[u], cc[u]);
            if (p >= 0) return p;
          }
        }
        return -1;
      } else {
        int64_t p = from;
        while (p + sl <= L && !eq(p)) ++p;
        return p + sl <= L ? p : -1;
      }
    };
    if (sg == 0 && anchor_start) {
      r = cur + sl <= L && eq(cur);
      cur += sl;
    } else if (last && anchor_end) {
      r = L - sl >= cur && eq(L - sl);
      cur = L;
    } else {
      const int64_t p = find(cur);
      r = p >= 0;
      cur = p + sl;
    }
  }
  if (r && anchor_end && (nseg == 0 || (nseg == 1 && anchor_start))) r = cur == L;
  return r;
}

// BLOCK threads take BLOCK consecutive strings per tile of at most TILE bytes.
// BLOCK = 64 makes every wave its own workgroup: the three tile barriers are
// single-wave barriers, and a wave waiting on its tile's loads never holds up
// the three others' matching (the 256-thread shape syncs all four per tile).
template <int BLOCK, int TILE, int SEGS = kSegMax>
__global__ __launch_bounds__(BLOCK) void like_seg_kernel(const int64_t* __restrict__ off,
                                                         const uint8_t* __restrict__ chars, int64_t n,
                                                         const uint8_t* __restrict__ seg, const int32_t* seg_off,
                                                         int nseg, bool anchor_start, bool anchor_end, bool negate,
                                                         uint8_t* __restrict__ out) {
  constexpr int kSegBits = TILE / 64;  // 64-bit words per segment bitmap
  __shared__ __attribute__((aligned(16))) uint8_t buf[TILE + 64];
  __shared__ uint64_t bits[SEGS][kSegBits];
  __shared__ uint8_t sseg[kLikeMaxPattern];
  __shared__ int32_t soff[SEGS + 1];
  const int total = seg_off[nseg];
  for (int i = threadIdx.x; i < total; i += BLOCK) sseg[i] = seg[i];
  if (threadIdx.x <= nseg) soff[threadIdx.x] = seg_off[threadIdx.x];
  const int64_t tiles = (n + BLOCK - 1) / BLOCK;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i0 = t * BLOCK;
    const int64_t i1 = i0 + BLOCK < n ? i0 + BLOCK : n;
    const uintptr_t lo = (uintptr_t)(chars + off[i0]);
    const uintptr_t hi = (uintptr_t)(chars + off[i1]);
    const uintptr_t start = lo & ~(uintptr_t)15;
    const uintptr_t full_end = hi & ~(uintptr_t)15;
    const int len = (int)(hi - start);
    const bool staged = hi - start <= (uintptr_t)TILE;
    __syncthreads();  // previous tile done; pattern visible on the first pass
    if (staged) {
      const int64_t nvec = (int64_t)(full_end - start) / 16;
      for (int64_t v = threadIdx.x; v < nvec; v += BLOCK) *(uint4*)(buf + v * 16) = *(const uint4*)(start + v * 16);
      for (uintptr_t a = full_end + threadIdx.x; a < hi; a += BLOCK) buf[a - start] = *(const uint8_t*)a;
      if (threadIdx.x < 64) buf[len + threadIdx.x] = 0;  // pad: comparisons may read past the tile end
      __syncthreads();
      // each lane tests the 16 positions of one 16-byte chunk against every
      // segment's 4-byte prefix in registers (v_alignbyte windows), verifies
      // the rare candidates byte-wise, and stores a 16-bit hit mask
      const int nchunks = ((len + 63) >> 6) * 4;
      for (int j = threadIdx.x; j < nchunks; j += BLOCK) {
        const uint4 v = *(const uint4*)(buf + j * 16);
        const uint32_t d[5] = {v.x, v.y, v.z, v.w, *(const uint32_t*)(buf + j * 16 + 16)};
        for (int sg = 0; sg < nseg; ++sg) {
          const int s0 = soff[sg], sl = soff[sg + 1] - s0;
          const int pl = sl < 4 ? sl : 4;
          uint32_t pref = 0;
          for (int k = 0; k < pl; ++k) pref |= (uint32_t)sseg[s0 + k] << (8 * k);
          const uint32_t pmask = pl == 4 ? 0xffffffffu : ((1u << (8 * pl)) - 1);
          uint32_t m = 0;
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const uint32_t w = __builtin_amdgcn_alignbyte(d[(q >> 2) + 1], d[q >> 2], q & 3);
            m |= (uint32_t)((w & pmask) == pref) << q;
          }
          const int base = j * 16;
          const int room = len - sl - base + 1;  // positions base+q with q < room fit in the tile
          m &= room >= 16 ? 0xffffu : room <= 0 ? 0u : ((1u << room) - 1);
          if (sl > 4) {
            for (uint32_t c = m; c; c &= c - 1) {
              const int q = __builtin_ctz(c);
              for (int k = 4; k < sl; ++k)
                if (buf[base + q + k] != sseg[s0 + k]) {
                  m &= ~(1u << q);
                  break;
                }
            }
          }
          ((uint16_t*)bits[sg])[j] = (uint16_t)m;
        }
      }
    }
    __syncthreads();
    const int64_t i = i0 + threadIdx.x;
    if (i < i1) {
      const int64_t a = off[i], e = off[i + 1];
      const bool r = staged ? seg_walk(bits, soff, nseg, anchor_start, anchor_end,
                                       (int)((uintptr_t)(chars + a) - start), (int)((uintptr_t)(chars + e) - start))
                            : seg_search<false>(chars + a, e - a, sseg, soff, nseg, anchor_start, anchor_end);
      out[i] = r != negate;
    }
  }
}

// Segments of >= 7 bytes ('%special%requests%', '%Customer%Complaints%'):
// the column is scanned as one byte stream and row structure is touched only
// where a candidate appears.
//
// Prefilter. Every occurrence of a segment at position p contains the aligned
// dword at a = p rounded up to 4, and that dword equals the segment's bytes
// a-p .. a-p+3 (a-p < 4, a-p+3 <= 6 < length). So a row can only match if one
// of its aligned dwords equals one of the 4 leading dword windows of a
// segment, and since every match contains every segment, testing the longest
// one is enough: 16 plain compares per 16-byte chunk. The row that holds an
// occurrence holds that dword, so the rows that intersect a passing chunk are
// the only ones that can match.
//
// A workgroup takes tiles of kLikeStreamRows consecutive rows. Per tile it
// reads the two offsets that bound the tile's bytes (one tile ahead), then
//   1. scans the 16-byte aligned chunks covering those bytes straight from
//      global memory, kLikeStreamChunks loads per lane in flight, no LDS
//      staging, no barrier, no limit on the tile's bytes; a lane whose chunk
//      passes appends the chunk's index to an LDS list;
//   2. resolves each listed chunk: the first of the tile's rows that
//      intersects it (from the offsets of every 64th row, kept in LDS, and two
//      rounds of independent loads), then the exact matcher (seg_search<true>:
//      greedy order, both anchors, a few rounds of wide loads per row) on that
//      row and the following ones that start inside the chunk; a match sets
//      the row's bit in an LDS bitmap. When the list overflows, every row of
//      the tile goes through the exact matcher instead: correct for any
//      input, fast for the usual one where candidates are rare;
//   3. writes out[i] = bit != negate for the tile's rows, 32 per lane.
// The kernel is left at the registers it asks for (about 107 VGPRs, 4 waves
// per SIMD): held to 8 waves it reloads spills inside the scan loop, and
// fewer resident waves also stream faster (profiles/like_stream_ab.txt, where
// the other tile sizes, load depths and a double-buffered scan are recorded).
// The first chunk of a tile is aligned down and the last one runs past the
// tile's end, so neighbouring tiles scan a shared chunk twice, but a
// workgroup resolves and writes only rows of its own tile, each exactly once.
// Nothing survives the launch and workgroups do not communicate.
constexpr int kLikeStreamRows = 4096;    // rows per tile: a multiple of 32
constexpr int kLikeStreamChunks = 4;     // 16-byte loads per lane in flight
constexpr int kLikeStreamStep = 64;      // rows between the offsets sampled into LDS for the resolve
static_assert(kLikeStreamRows % 32 == 0 && kLikeStreamRows / kLikeStreamStep <= kBlock, "tile shape");
constexpr int kLikeStreamCand = 2048;    // listed chunks per tile; with more (over one per two rows) the tile takes every row

template <int kU>
__global__ __launch_bounds__(kBlock) void like_stream_kernel(const int64_t* __restrict__ off,
                                                            const uint8_t* __restrict__ chars, int64_t n,
                                                            const uint8_t* __restrict__ seg, const int32_t* seg_off,
                                                            int nseg, bool anchor_start, bool anchor_end, bool negate,
                                                            uint8_t* __restrict__ out, int64_t nbytes) {
  constexpr int R = kLikeStreamRows;
  __shared__ uint32_t cand[kLikeStreamCand];
  __shared__ uint32_t hit[R / 32];
  __shared__ uint32_t ncand[2];   // by tile parity: reset two barriers before its next use
  __shared__ int64_t samp[R / kLikeStreamStep];   // the offset of every 64th row of the tile
  __shared__ uint8_t sseg[kLikeMaxPattern];
  __shared__ int32_t soff[kSegMax + 1];
  const int tid = threadIdx.x;
  const int total = seg_off[nseg];
  for (int i = tid; i < total; i += kBlock) sseg[i] = seg[i];
  if (tid <= nseg) soff[tid] = seg_off[tid];
  for (int w = tid; w < R / 32; w += kBlock) hit[w] = 0;
  if (tid < 2) ncand[tid] = 0;
  __syncthreads();
  // the 4 leading dword windows of the longest segment, wave-uniform: kept in
  // scalar registers (compares take an SGPR operand)
  int f0 = soff[0];
  for (int sg = 1, best = soff[1] - soff[0]; sg < nseg; ++sg)
    if (soff[sg + 1] - soff[sg] > best) {
      best = soff[sg + 1] - soff[sg];
      f0 = soff[sg];
    }
  uint32_t P[4];
#pragma unroll
  for (int o = 0; o < 4; ++o)
    P[o] = __builtin_amdgcn_readfirstlane((uint32_t)sseg[f0 + o] | ((uint32_t)sseg[f0 + o + 1] << 8) |
                                          ((uint32_t)sseg[f0 + o + 2] << 16) | ((uint32_t)sseg[f0 + o + 3] << 24));
  // some dword equals some window <=> the smallest of the 16 xors is 0
  // (v_xor + v_min3: no per-compare mask bookkeeping)
  auto passes = [&](const uint4& v) {
    uint32_t m = ~0u;
#pragma unroll
    for (int o = 0; o < 4; ++o) m = min(min(m, v.x ^ P[o]), min(min(v.y ^ P[o], v.z ^ P[o]), v.w ^ P[o]));
    return m == 0;
  };
  const uint8_t* const chars_end = chars + nbytes;
  const bool out16 = ((uintptr_t)out & 15) == 0;
  const uint32_t flip = negate ? 0x01010101u : 0u;
  const int64_t tiles = (n + R - 1) / R;
  // the tile's byte range is known one tile ahead (no offsets -> chars load chain)
  int64_t t_lo = 0, t_hi = 0;
  if ((int64_t)blockIdx.x < tiles) {
    const int64_t r0 = (int64_t)blockIdx.x * R;
    t_lo = off[r0];
    t_hi = off[r0 + R < n ? r0 + R : n];
  }
  int par = 0;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x, par ^= 1) {
    const int64_t i0 = t * R;
    const int64_t i1 = i0 + R < n ? i0 + R : n;
    const int64_t lo = t_lo, hi = t_hi;
    {
      const int64_t tn = t + gridDim.x;
      if (tn < tiles) {
        const int64_t r0 = tn * R;
        t_lo = off[r0];
        t_hi = off[r0 + R < n ? r0 + R : n];
      }
    }
    // chunk j is the 16 bytes at position pos0 + 16 j of the buffer, 16-byte aligned in memory
    const int64_t pos0 = lo - (int64_t)((uintptr_t)(chars + lo) & 15);
    const int64_t nchunks = hi > lo ? (hi - pos0 + 15) >> 4 : 0;
    // chunks [jv0, jv1) lie wholly inside the buffer; the others (at most the
    // first and the last) are read byte by byte, never outside [chars, chars_end)
    const int64_t jv0 = pos0 < 0 ? 1 : 0;
    const int64_t jv1 = (nbytes - pos0) >> 4;
    const bool listed = nchunks <= 0xffffffffLL;   // chunk indices are kept in 32 bits
    // sampled offsets for the resolve: loaded now, needed only after the scan
    const bool sampler = i0 + (int64_t)tid * kLikeStreamStep < i1 && tid < R / kLikeStreamStep;
    const int64_t sample = sampler ? off[i0 + (int64_t)tid * kLikeStreamStep] : 0;
    auto load = [&](int64_t j) {
      if (j >= jv0 && j < jv1) return *(const uint4*)(chars + (pos0 + 16 * j));
      uint32_t d[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        uint32_t x = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint8_t* p = chars + (pos0 + 16 * j + 4 * w + k);
          if (p >= chars && p < chars_end) x |= (uint32_t)*p << (8 * k);
        }
        d[w] = x;
      }
      return uint4{d[0], d[1], d[2], d[3]};
    };
    auto append = [&](int64_t j) {
      const uint32_t c = atomicAdd(&ncand[par], 1u);
      if (c < (uint32_t)kLikeStreamCand) cand[c] = (uint32_t)j;
    };
    if (listed) {
      for (int64_t j0 = 0; j0 < nchunks; j0 += kU * kBlock) {
        uint4 v[kU];
        if (j0 >= jv0 && j0 + kU * kBlock <= (nchunks < jv1 ? nchunks : jv1)) {   // uniform: all loads, then all compares
#pragma unroll
          for (int u = 0; u < kU; ++u) v[u] = *(const uint4*)(chars + (pos0 + 16 * (j0 + u * kBlock + tid)));
#pragma unroll
          for (int u = 0; u < kU; ++u)
            if (passes(v[u])) append(j0 + u * kBlock + tid);
        } else {
#pragma unroll
          for (int u = 0; u < kU; ++u) {
            const int64_t j = j0 + u * kBlock + tid;
            if (j < nchunks && passes(load(j))) append(j);
          }
        }
      }
    }
    if (sampler) samp[tid] = sample;
    __syncthreads();
    auto test_row = [&](int64_t r) {
      const int64_t a = off[r], e = off[r + 1];
      if (seg_search<true>(chars + a, e - a, sseg, soff, nseg, anchor_start, anchor_end))
        atomicOr(&hit[(r - i0) >> 5], 1u << ((r - i0) & 31));
    };
    const uint32_t nc = ncand[par];
    if (listed && nc <= (uint32_t)kLikeStreamCand) {
      for (uint32_t c = tid; c < nc; c += kBlock) {
        const int64_t b = pos0 + 16 * (int64_t)cand[c];
        const int64_t first = b > lo ? b : lo;              // in [lo, hi): the chunk intersects the tile
        const int64_t end = b + 16 < hi ? b + 16 : hi;
        // the last row of the tile that starts at or before `first` holds that
        // byte (rows before it that start there too are empty). Every load of
        // an offset waits a full trip through a busy memory system, so: the
        // group of 64 rows from the samples in LDS, then two rounds of seven
        // loads that do not wait for each other (every 8th row, then every
        // row). Offsets past the group are larger than `first` already; off[i1] is.
        int k = 0, ke = (int)((i1 - i0 + kLikeStreamStep - 1) / kLikeStreamStep);
        while (ke - k > 1) {
          const int mid = (k + ke) >> 1;
          if (samp[mid] <= first) k = mid;
          else ke = mid;
        }
        int64_t r = i0 + (int64_t)k * kLikeStreamStep;
#pragma unroll
        for (int step = 8; step; step >>= 3) {
          int64_t x[7];
#pragma unroll
          for (int q = 0; q < 7; ++q) x[q] = off[r + (q + 1) * step < i1 ? r + (q + 1) * step : i1];
          int cnt = 0;
#pragma unroll
          for (int q = 0; q < 7; ++q) cnt += x[q] <= first;
          r += cnt * step;
        }
        for (; r < i1 && off[r] < end; ++r) test_row(r);
      }
    } else {
      for (int64_t r = i0 + tid; r < i1; r += kBlock) test_row(r);
    }
    __syncthreads();
    if (tid == 0) ncand[par] = 0;
    for (int w = tid; w < R / 32; w += kBlock) {
      const uint32_t bits = hit[w];
      if (bits) hit[w] = 0;
      const int64_t r0 = i0 + 32 * w;
      if (out16 && r0 + 32 <= i1) {
        uint32_t d[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) d[q] = ((((bits >> (4 * q)) & 15u) * 0x00204081u) & 0x01010101u) ^ flip;   // 4 bits -> 4 bytes
        *(uint4*)(out + r0) = uint4{d[0], d[1], d[2], d[3]};
        *(uint4*)(out + r0 + 16) = uint4{d[4], d[5], d[6], d[7]};
      } else {
        for (int k = 0; k < 32 && r0 + k < i1; ++k) out[r0 + k] = (uint8_t)(((bits >> k) & 1u) ^ (negate ? 1u : 0u));
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void case_kernel(const uint8_t* __restrict__ in, int64_t nbytes, bool to_upper,
                                                     uint8_t* __restrict__ out, int* __restrict__ non_ascii) {
  int found = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nbytes; i += (int64_t)gridDim.x * blockDim.x) {
    uint8_t c = in[i];
    found |= c >= 0x80;
    if (to_upper) c = (c >= 'a' && c <= 'z') ? c - 32 : c;
    else c = (c >= 'A' && c <= 'Z') ? c + 32 : c;
    out[i] = c;
  }
  if (__any(found) && lane_id() == 0) atomicOr(non_ascii, 1);
}

// byte range [b, e) of characters [start, start+len) (1-based SQL semantics)
__device__ inline void substr_range(const uint8_t* s, int64_t n, int64_t start, int64_t len, bool has_len,
                                    int64_t* b, int64_t* e) {
  // SQL: characters from position start (1-based); start<1 shortens len
  int64_t first = start, last;  // character positions (1-based, inclusive/exclusive)
  if (has_len) {
    last = start + len;  // exclusive
    if (len < 0) last = start;
  } else {
    last = INT64_MAX;
  }
  if (first < 1) first = 1;
  int64_t pos = 1, byte = 0;
  int64_t bb = n, ee = n;
  while (byte < n) {
    if (pos == first) bb = byte;
    if (pos == last) { ee = byte; break; }
    // advance one UTF-8 character
    ++byte;
    while (byte < n && (s[byte] & 0xC0) == 0x80) ++byte;
    ++pos;
  }
  if (bb > ee) bb = ee;
  if (last <= first) bb = ee = (bb < n ? bb : n);
  *b = bb;
  *e = ee;
}

__global__ __launch_bounds__(kBlock) void substr_len_kernel(const int64_t* __restrict__ off, const uint8_t* __restrict__ chars,
                                                           int64_t n, int64_t start, int64_t len, bool has_len,
                                                           int64_t* __restrict__ out_len) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = off[i], b, e;
    substr_range(chars + a, off[i + 1] - a, start, len, has_len, &b, &e);
    out_len[i] = e - b;
  }
}

__global__ __launch_bounds__(kBlock) void substr_copy_kernel(const int64_t* __restrict__ off, const uint8_t* __restrict__ chars,
                                                            int64_t n, int64_t start, int64_t len, bool has_len,
                                                            const int64_t* __restrict__ new_off, uint8_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = off[i], b, e;
    substr_range(chars + a, off[i + 1] - a, start, len, has_len, &b, &e);
    int64_t d = new_off[i];
    for (int64_t k = b; k < e; ++k) out[d + k - b] = chars[a + k];
  }
}

__device__ inline uint64_t hash_bytes(const uint8_t* s, int64_t n) {
  uint64_t h = 0x9E3779B97F4A7C15ULL ^ (uint64_t)n;
  int64_t k = 0;
  for (; k + 8 <= n; k += 8) {
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) w |= (uint64_t)s[k + j] << (8 * j);
    h = mix64(h ^ w) + 0x632BE59BD9B4E019ULL;
  }
  uint64_t w = 0;
  for (int j = 0; k + j < n; ++j) w |= (uint64_t)s[k + j] << (8 * j);
  return mix64(h ^ w ^ 0xA0761D6478BD642FULL);
}

__global__ __launch_bounds__(kBlock) void hash_kernel(const int64_t* __restrict__ off, const uint8_t* __restrict__ chars,
                                                     int64_t n, const uint8_t* __restrict__ valid, int64_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (valid && !valid[i]) { out[i] = 0x7fffffffffffff00LL; continue; }
    int64_t a = off[i];
    uint64_t h = hash_bytes(chars + a, off[i + 1] - a);
    if ((int64_t)h == kEmptyKey) h ^= 1;  // keep clear of the hash-table sentinel
    out[i] = (int64_t)h;
  }
}

__device__ inline int cmp_bytes(const uint8_t* a, int64_t na, const uint8_t* b, int64_t nb) {
  int64_t m = na < nb ? na : nb;
  for (int64_t k = 0; k < m; ++k) {
    if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
  }
  return na == nb ? 0 : (na < nb ? -1 : 1);
}

template <typename I>
__global__ __launch_bounds__(kBlock) void eq_rows_kernel(const int64_t* __restrict__ aoff, const uint8_t* __restrict__ achars,
                                                        const I* __restrict__ ai, const int64_t* __restrict__ boff,
                                                        const uint8_t* __restrict__ bchars, const I* __restrict__ bi,
                                                        int64_t n, int* __restrict__ mismatches) {
  int bad = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t x = ai ? (int64_t)ai[i] : i, y = bi ? (int64_t)bi[i] : i;
    int64_t a0 = aoff[x], b0 = boff[y];
    bad |= cmp_bytes(achars + a0, aoff[x + 1] - a0, bchars + b0, boff[y + 1] - b0) != 0;
  }
  if (__any(bad) && lane_id() == 0) atomicAdd(mismatches, 1);
}

// op: 0 '=', 1 '<>', 2 '<', 3 '<=', 4 '>', 5 '>='
__global__ __launch_bounds__(kBlock) void cmp_const_kernel(const int64_t* __restrict__ off, const uint8_t* __restrict__ chars,
                                                          int64_t n, const uint8_t* __restrict__ c, int64_t cn, int op,
                                                          uint8_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = off[i];
    int r = cmp_bytes(chars + a, off[i + 1] - a, c, cn);
    bool v;
    switch (op) {
      case 0: v = r == 0; break;
      case 1: v = r != 0; break;
      case 2: v = r < 0; break;
      case 3: v = r <= 0; break;
      case 4: v = r > 0; break;
      default: v = r >= 0; break;
    }
    out[i] = v;
  }
}

// String IN (constants) in one pass: row i is set when its bytes equal one of
// the nv constants vb[voff[v] .. voff[v+1]) -- or, with vmode[v] = 1, start
// with them (substr(x, 1, L) IN (...) for a constant of exactly L code points;
// UTF-8 is self-synchronising, so a byte prefix of L code points is the
// substring). Replaces one compare pass per constant plus the substring copy
// (TPC-H Q22's country codes: 7 passes over 15M phone numbers).
constexpr int kInSetWords = 256;   // constants staged in LDS as words

__global__ __launch_bounds__(kBlock) void in_set_kernel(const int64_t* __restrict__ off,
                                                       const uint8_t* __restrict__ chars, int64_t n,
                                                       const uint8_t* __restrict__ vb, const int32_t* __restrict__ voff,
                                                       const uint8_t* __restrict__ vmode, int nv,
                                                       uint8_t* __restrict__ out) {
  // constants of at most 8 bytes (the usual case: codes, flags, short names)
  // compare as masked words against the row's first bytes, loaded once; the
  // constants' words, lengths and modes are built once per workgroup in LDS
  // (not re-read byte by byte from global memory for every row)
  __shared__ uint64_t cword[kInSetWords];
  __shared__ int32_t clen[kInSetWords];
  int maxb = 0;
  for (int v = 0; v < nv; ++v) maxb = max(maxb, voff[v + 1] - voff[v]);
  const bool words = maxb <= 8;
  const bool staged = words && nv <= kInSetWords;
  if (staged) {
    for (int v = threadIdx.x; v < nv; v += blockDim.x) {
      const int32_t c0 = voff[v], vl = voff[v + 1] - c0;
      uint64_t cw = 0;
      for (int32_t j = 0; j < vl; ++j) cw |= (uint64_t)vb[c0 + j] << (8 * j);
      cword[v] = cw;
      clen[v] = vmode[v] ? -vl - 1 : vl;   // negative: prefix match of length -clen-1
    }
    __syncthreads();
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = off[i], len = off[i + 1] - a;
    bool hit = false;
    if (staged) {
      const int nb = len < maxb ? (int)len : maxb;
      uint64_t w = 0;
      for (int j = 0; j < nb; ++j) w |= (uint64_t)chars[a + j] << (8 * j);
      for (int v = 0; v < nv && !hit; ++v) {
        const int32_t cl = clen[v];
        const int32_t vl = cl < 0 ? -cl - 1 : cl;
        if (cl < 0 ? len < vl : len != vl) continue;
        const uint64_t m = vl >= 8 ? ~0ull : ((1ull << (8 * vl)) - 1);
        hit = (w & m) == cword[v];
      }
    } else if (words) {
      const int nb = len < maxb ? (int)len : maxb;
      uint64_t w = 0;
      for (int j = 0; j < nb; ++j) w |= (uint64_t)chars[a + j] << (8 * j);
      for (int v = 0; v < nv && !hit; ++v) {
        const int32_t c0 = voff[v], vl = voff[v + 1] - c0;
        if (vmode[v] ? len < vl : len != vl) continue;
        uint64_t cw = 0;
        for (int32_t j = 0; j < vl; ++j) cw |= (uint64_t)vb[c0 + j] << (8 * j);
        const uint64_t m = vl >= 8 ? ~0ull : ((1ull << (8 * vl)) - 1);
        hit = (w & m) == cw;
      }
    } else {
      for (int v = 0; v < nv && !hit; ++v) {
        const int32_t c0 = voff[v], vl = voff[v + 1] - c0;
        if (vmode[v] ? len < vl : len != vl) continue;
        bool eq = true;
        for (int32_t j = 0; j < vl && eq; ++j) eq = chars[a + j] == vb[c0 + j];
        hit = eq;
      }
    }
    out[i] = hit;
  }
}

// 8-byte big-endian prefix as an order-preserving uint64 (minus sign flip):
// first sort key for ORDER BY on strings.
__global__ __launch_bounds__(kBlock) void prefix_key_kernel(const int64_t* __restrict__ off, const uint8_t* __restrict__ chars,
                                                           int64_t n, int64_t skip, int64_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = off[i] + skip, e = off[i + 1];
    uint64_t k = 0;
    for (int j = 0; j < 8; ++j) k = (k << 8) | (a + j < e ? chars[a + j] : 0);
    out[i] = (int64_t)(k ^ 0x8000000000000000ULL);
  }
}

}  // namespace

void str_like(const int64_t* off, const uint8_t* chars, int64_t n, const uint8_t* pat, const uint8_t* kind, int m,
              bool case_insensitive, bool negate, uint8_t* out, hipStream_t stream) {
  if (n == 0) return;
  if (m <= kLikeMaxPattern)
    hipLaunchKernelGGL(like_tile_kernel, dim3(grid_for(n, kBlock, 256 * 8 * 4)), dim3(kBlock), 0, stream, off, chars, n,
                       pat, kind, m, case_insensitive, negate, out);
  else
    hipLaunchKernelGGL(like_kernel, dim3(grid_for(n, kBlock, 65536)), dim3(kBlock), 0, stream, off, chars, n, pat, kind,
                       m, case_insensitive, negate, out);
  check_launch("str_like", stream);
}

void str_like_segments(const int64_t* off, const uint8_t* chars, int64_t n, const uint8_t* seg, const int32_t* seg_off,
                       int nseg, bool anchor_start, bool anchor_end, bool negate, uint8_t* out, int64_t nbytes,
                       int min_seg, hipStream_t stream) {
  if (n == 0) return;
  if (nseg > kSegMax) throw std::runtime_error("str_like_segments: too many segments");
  const bool dword_filter = !debug_flag("like_nodword");
  if (dword_filter && nseg >= 1 && nseg <= 2 && min_seg >= 7) {
    // 8 workgroups per CU, half of them resident at a time, each walking
    // several tiles (like_few_wgs: two workgroups, so that a test-sized column
    // gives each many tiles)
    const int64_t max_wgs = debug_flag("like_few_wgs") ? 2 : 256 * 8;
    hipLaunchKernelGGL((like_stream_kernel<kLikeStreamChunks>), dim3(grid_for(n, kLikeStreamRows, max_wgs)), dim3(kBlock),
                       0, stream, off, chars, n, seg, seg_off, nseg, anchor_start, anchor_end, negate, out, nbytes);
    check_launch("str_like_segments", stream);
    return;
  }
  // like_seg_kernel. (a one-wave-per-workgroup variant with 4 / 8 KB tiles
  // measured slower for Q13 at SF100, 14.6 vs 11.7 ms per query:
  // profiles/r3_ab_like_wave.txt)
  // one or two segments (nearly every analytic LIKE): a bitmap sized for
  // them frees 4-6 KB of LDS per workgroup, one or two more resident
  // workgroups per CU (-9 % / -10 % for two / one segment,
  // profiles/r4_select_like_ab.txt)
  if (nseg <= 1)
    hipLaunchKernelGGL((like_seg_kernel<kBlock, kLikeTileBytes, 1>), dim3(grid_for(n, kBlock, 256 * 8 * 4)),
                       dim3(kBlock), 0, stream, off, chars, n, seg, seg_off, nseg, anchor_start, anchor_end, negate, out);
  else if (nseg <= 2)
    hipLaunchKernelGGL((like_seg_kernel<kBlock, kLikeTileBytes, 2>), dim3(grid_for(n, kBlock, 256 * 8 * 4)),
                       dim3(kBlock), 0, stream, off, chars, n, seg, seg_off, nseg, anchor_start, anchor_end, negate, out);
  else
    hipLaunchKernelGGL((like_seg_kernel<kBlock, kLikeTileBytes>), dim3(grid_for(n, kBlock, 256 * 8 * 4)), dim3(kBlock),
                       0, stream, off, chars, n, seg, seg_off, nseg, anchor_start, anchor_end, negate, out);
  check_launch("str_like_segments", stream);
}

void str_case(const uint8_t* in, int64_t nbytes, bool to_upper, uint8_t* out, int* non_ascii, hipStream_t stream) {
  if (nbytes == 0) return;
  hipLaunchKernelGGL(case_kernel, dim3(grid_for(nbytes, kBlock, 65536)), dim3(kBlock), 0, stream, in, nbytes, to_upper,
                     out, non_ascii);
  check_launch("str_case", stream);
}

void str_substr_lengths(const int64_t* off, const uint8_t* chars, int64_t n, int64_t start, int64_t len, bool has_len,
                        int64_t* out_len, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(substr_len_kernel, dim3(grid_for(n, kBlock, 65536)), dim3(kBlock), 0, stream, off, chars, n, start,
                     len, has_len, out_len);
  check_launch("str_substr_lengths", stream);
}

void str_substr_copy(const int64_t* off, const uint8_t* chars, int64_t n, int64_t start, int64_t len, bool has_len,
                     const int64_t* new_off, uint8_t* out, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(substr_copy_kernel, dim3(grid_for(n, kBlock, 65536)), dim3(kBlock), 0, stream, off, chars, n, start,
                     len, has_len, new_off, out);
  check_launch("str_substr_copy", stream);
}

// Order-preserving 8-byte chunks of each string: out[k * n + i] holds bytes
// [8k, 8k + 8) of string i big-endian, zero padded (a shorter string sorts
// first on a common prefix, as in byte-wise UTF-8 order), sign bit flipped so
// signed int64 order equals unsigned byte order. An LSD sort over the chunks
// (last chunk first) orders the strings: ops/strings.py sort_ranks.
__global__ __launch_bounds__(kBlock) void prefix_keys_kernel(const int64_t* __restrict__ off,
                                                             const uint8_t* __restrict__ chars, int64_t n,
                                                             int chunks, int64_t* __restrict__ out) {
  const int64_t total = n * chunks;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = t / n, i = t - k * n;
    const int64_t a = off[i], len = off[i + 1] - a, b0 = 8 * k;
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t p = b0 + j;
      v = (v << 8) | (p < len ? (uint64_t)chars[a + p] : 0u);
    }
    out[t] = (int64_t)(v ^ 0x8000000000000000ull);
  }
}

void str_prefix_keys(const int64_t* off, const uint8_t* chars, int64_t n, int chunks, int64_t* out,
                     hipStream_t stream) {
  if (n == 0 || chunks <= 0) return;
  hipLaunchKernelGGL(prefix_keys_kernel, dim3(grid_for(n * chunks, kBlock, 65536)), dim3(kBlock), 0, stream, off,
                     chars, n, chunks, out);
  check_launch("str_prefix_keys", stream);
}

void str_hash64(const int64_t* off, const uint8_t* chars, int64_t n, const uint8_t* valid, int64_t* out,
                hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(hash_kernel, dim3(grid_for(n, kBlock, 65536)), dim3(kBlock), 0, stream, off, chars, n, valid, out);
  check_launch("str_hash64", stream);
}

void str_eq_rows(const int64_t* aoff, const uint8_t* achars, const void* ai, const int64_t* boff, const uint8_t* bchars,
                 const void* bi, bool idx64, int64_t n, int* mismatches, hipStream_t stream) {
  if (n == 0) return;
  dim3 g(grid_for(n, kBlock, 65536)), b(kBlock);
  dispatch(wide{idx64}, [&](auto i) {
    using I = type_of<decltype(i)>;
    launch("str_eq_rows", eq_rows_kernel<I>, g, b, 0, stream, aoff, achars, as<I>(ai), boff, bchars, as<I>(bi), n,
           mismatches);
  });
}

void str_cmp_const(const int64_t* off, const uint8_t* chars, int64_t n, const uint8_t* c, int64_t cn, int op,
                   uint8_t* out, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(cmp_const_kernel, dim3(grid_for(n, kBlock, 65536)), dim3(kBlock), 0, stream, off, chars, n, c, cn,
                     op, out);
  check_launch("str_cmp_const", stream);
}

void str_in_set(const int64_t* off, const uint8_t* chars, int64_t n, const uint8_t* vb, const int32_t* voff,
                const uint8_t* vmode, int nv, uint8_t* out, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(in_set_kernel, dim3(grid_for(n, kBlock, 65536)), dim3(kBlock), 0, stream, off, chars, n, vb, voff,
                     vmode, nv, out);
  check_launch("str_in_set", stream);
}

void str_prefix_key(const int64_t* off, const uint8_t* chars, int64_t n, int64_t skip, int64_t* out,
                    hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(prefix_key_kernel, dim3(grid_for(n, kBlock, 65536)), dim3(kBlock), 0, stream, off, chars, n, skip,
                     out);
  check_launch("str_prefix_key", stream);
}

}  // namespace kern
}  // namespace igloo
