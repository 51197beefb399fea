// Byte-string (BINARY) functions: encode / decode in hex and base64, and the
// UTF-8 validation behind CAST(binary AS VARCHAR).
//
// hex: no scan. Output offsets are the input offsets times two (encode) or
//   halved (decode), and output byte 2k, 2k+1 depends on input byte k alone,
//   so both directions are flat byte streams: a lane takes 8 (encode) or 16
//   (decode) input bytes with one load and writes 16 or 8 bytes with one
//   store; the last bytes that do not fill a group go one byte per lane.
//   The flat decode writer is right only for dense, even rows. Rows of one
//   offsets array are dense by construction; a column whose offsets do not
//   start at 0 is handled in the kernel (it reads from chars + off[0], the
//   caller rebases the halved offsets); NULL rows that hold bytes, which
//   may be odd, are flagged by the validator and the caller (ops/binary.py)
//   empties them with one gather first.
// base64: lengths, the existing offsets scan, then a cooperative writer. A
//   block stages the input and output offsets of a tile of kB64Tile rows in
//   LDS and its lanes own aligned 8-byte chunks of the tile's *output* range:
//   lane t writes bytes [8t, 8t+8) with one store, finding the row of its
//   first byte by a binary search of the staged offsets and stepping rows
//   from there. Chosen over "a wave per row" because rows of 8..64 bytes
//   would leave most of a wave idle (a 12-byte row has 4 groups for 64
//   lanes), while chunk ownership keeps every lane busy at any row length
//   and makes neighbouring lanes store neighbouring bytes. Only the two
//   chunks at the ends of a tile's range are clipped and written bytewise.
// validation: hex and base64 validators are one launch each that covers two
//   domains: a flat pass over bytes (a lane checks 8 bytes; on a bad byte it
//   finds the row by binary search and skips NULL rows) and a pass over rows
//   (odd length / padding / trailing bits / output length). The smallest bad
//   row index lands in err[0] by atomicMin; the host reads it back once.
// utf8: pass 1 ORs the high bits of 4 KiB tiles into one flag byte per tile
//   (a streaming pass, all an ASCII column costs besides a flag read per
//   row); pass 2 runs the per-row automaton only on rows that touch a
//   flagged tile. Each row is validated on its own.
#include "common.h"
#include "kernels.h"

namespace igloo {
namespace kern {

namespace {

constexpr int kUtf8Tile = kBlock * 16;   // bytes per high-bit flag

__device__ __forceinline__ int hex_val(uint8_t c) {
  if (c >= '0' && c <= '9') return c - '0';
  const uint8_t l = c | 0x20;
  if (l >= 'a' && l <= 'f') return l - 'a' + 10;
  return -1;
}

__device__ __forceinline__ int b64_val(uint8_t c) {
  if (c >= 'A' && c <= 'Z') return c - 'A';
  if (c >= 'a' && c <= 'z') return c - 'a' + 26;
  if (c >= '0' && c <= '9') return c - '0' + 52;
  if (c == '+') return 62;
  if (c == '/') return 63;
  return -1;
}

__device__ __forceinline__ uint8_t b64_chr(int v) {
  return (uint8_t)(v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '+' : '/');
}

// first row r of [0, nrows) with off[r + 1] > j: the row that holds byte j (empty rows are
// stepped over). Needs off[0] <= j < off[nrows].
__device__ __forceinline__ int64_t row_of(const int64_t* off, int64_t nrows, int64_t j) {
  int64_t lo = 0, hi = nrows - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid + 1] > j) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ void report_row(unsigned long long* err, const uint8_t* valid, int64_t r) {
  if (valid == nullptr || valid[r]) atomicMin(err, (unsigned long long)r);
}

// 4 bytes -> their 8 lowercase hex characters (memory order: high nibble first)
__device__ __forceinline__ uint64_t hex8(uint32_t x) {
  uint64_t t = x;
  t = (t | (t << 16)) & 0x0000FFFF0000FFFFull;
  t = (t | (t << 8)) & 0x00FF00FF00FF00FFull;
  const uint64_t nib = ((t >> 4) & 0x000F000F000F000Full) | ((t & 0x000F000F000F000Full) << 8);
  const uint64_t ge10 = ((nib + 0x0606060606060606ull) >> 4) & 0x0101010101010101ull;
  return nib + 0x3030303030303030ull + ge10 * 39;   // 'a' - '0' - 10
}

__device__ __forceinline__ void put_hex2(uint8_t* o, uint8_t v) {
  const uint8_t h = v >> 4, l = v & 15;
  o[0] = (uint8_t)(h < 10 ? '0' + h : 'a' + h - 10);
  o[1] = (uint8_t)(l < 10 ? '0' + l : 'a' + l - 10);
}

// ---------------------------------------------------------------- hex
__global__ __launch_bounds__(kBlock) void hex_encode_kernel(const uint8_t* __restrict__ in, int64_t nbytes,
                                                          uint8_t* __restrict__ out) {
  const int64_t groups = nbytes >> 3;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    uint64_t v;
    __builtin_memcpy(&v, in + 8 * g, 8);
    uint64_t o[2] = {hex8((uint32_t)v), hex8((uint32_t)(v >> 32))};
    __builtin_memcpy(out + 16 * g, o, 16);
  }
  const int64_t k = 8 * groups + threadIdx.x;      // the last nbytes % 8 bytes
  if (blockIdx.x == 0 && k < nbytes) put_hex2(out + 2 * k, in[k]);
}

// err[0]: smallest bad row (the caller sets it to n); err[1]: set when a NULL row holds bytes (the
// flat writer then needs them emptied first).
__global__ __launch_bounds__(kBlock) void hex_validate_kernel(const int64_t* __restrict__ off,
                                                            const uint8_t* __restrict__ chars,
                                                            const uint8_t* __restrict__ valid, int64_t n,
                                                            unsigned long long* __restrict__ err) {
  const int64_t base = off[0], nbytes = off[n] - base;
  const int64_t groups = (nbytes + 7) >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t g = first; g < groups; g += stride) {
    const int64_t j0 = base + 8 * g, cnt = nbytes - 8 * g < 8 ? nbytes - 8 * g : 8;
    uint64_t v = 0;
    if (cnt == 8) __builtin_memcpy(&v, chars + j0, 8);
    else for (int64_t k = 0; k < cnt; ++k) v |= (uint64_t)chars[j0 + k] << (8 * k);
    for (int64_t k = 0; k < cnt; ++k)
      if (hex_val((uint8_t)(v >> (8 * k))) < 0) report_row(err, valid, row_of(off, n, j0 + k));
  }
  for (int64_t r = first; r < n; r += stride) {
    const int64_t len = off[r + 1] - off[r];
    if (valid != nullptr && !valid[r]) {
      if (len) atomicMax(err + 1, 1ull);
    } else if (len & 1) {
      atomicMin(err, (unsigned long long)r);
    }
  }
}

// rows are dense and even: output byte k comes from input bytes off[0] + 2k, off[0] + 2k + 1
// (never more than out_cap bytes: the host sized out from a readback that a replay may hand back stale)
__global__ __launch_bounds__(kBlock) void hex_decode_kernel(const int64_t* __restrict__ off, int64_t n,
                                                          const uint8_t* __restrict__ in, int64_t out_cap,
                                                          uint8_t* __restrict__ out) {
  in += off[0];
  const int64_t want = (off[n] - off[0]) >> 1;
  const int64_t nout = want < out_cap ? want : out_cap;
  const int64_t groups = nout >> 3;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    uint64_t v[2];
    __builtin_memcpy(v, in + 16 * g, 16);
    uint64_t o = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint64_t w = v[k >> 2] >> (16 * (k & 3));
      o |= (uint64_t)(uint8_t)(((hex_val((uint8_t)w) & 15) << 4) | (hex_val((uint8_t)(w >> 8)) & 15)) << (8 * k);
    }
    __builtin_memcpy(out + 8 * g, &o, 8);
  }
  const int64_t k = 8 * groups + threadIdx.x;
  if (blockIdx.x == 0 && k < nout)
    out[k] = (uint8_t)(((hex_val(in[2 * k]) & 15) << 4) | (hex_val(in[2 * k + 1]) & 15));
}

// ---------------------------------------------------------------- base64
__global__ __launch_bounds__(kBlock) void b64_enc_lengths_kernel(const int64_t* __restrict__ off,
                                                               const uint8_t* __restrict__ valid, int64_t n,
                                                               int64_t* __restrict__ lens) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
    lens[r] = (valid != nullptr && !valid[r]) ? 0 : (4 * (off[r + 1] - off[r]) + 2) / 3;
}

// Output length of one row (unpadded or correctly padded base64), -1 when its shape is wrong:
// padding that does not complete a quantum, a length of 1 (mod 4) without it, non-zero trailing bits.
// Bytes outside the alphabet and a '=' before the end are the flat pass's to find.
__device__ __forceinline__ int64_t b64_row_outlen(const uint8_t* s, int64_t len) {
  int p = 0;
  if (len >= 1 && s[len - 1] == '=') p = (len >= 2 && s[len - 2] == '=') ? 2 : 1;
  const int64_t L = len - p;
  if (p && (len & 3)) return -1;
  if ((L & 3) == 1) return -1;
  if (L & 3) {
    const int v = b64_val(s[L - 1]);
    if (v >= 0 && (v & ((L & 3) == 2 ? 15 : 3))) return -1;
  }
  return L * 3 / 4;
}

// is byte j (in row r, rows [off[r], off[r+1])) acceptable?
__device__ __forceinline__ bool b64_byte_ok(const int64_t* off, const uint8_t* chars, int64_t r, int64_t j) {
  const uint8_t c = chars[j];
  if (b64_val(c) >= 0) return true;
  if (c != '=') return false;
  const int64_t end = off[r + 1];
  return j == end - 1 || (j == end - 2 && chars[end - 1] == '=');
}

__global__ __launch_bounds__(kBlock) void b64_dec_lengths_kernel(const int64_t* __restrict__ off,
                                                               const uint8_t* __restrict__ chars,
                                                               const uint8_t* __restrict__ valid, int64_t n,
                                                               int64_t* __restrict__ lens,
                                                               unsigned long long* __restrict__ err) {
  const int64_t base = off[0], nbytes = off[n] - base;
  const int64_t groups = (nbytes + 7) >> 3;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t g = first; g < groups; g += stride) {
    const int64_t j0 = base + 8 * g, cnt = nbytes - 8 * g < 8 ? nbytes - 8 * g : 8;
    uint64_t v = 0;
    if (cnt == 8) __builtin_memcpy(&v, chars + j0, 8);
    else for (int64_t k = 0; k < cnt; ++k) v |= (uint64_t)chars[j0 + k] << (8 * k);
    for (int64_t k = 0; k < cnt; ++k) {
      if (b64_val((uint8_t)(v >> (8 * k))) >= 0) continue;
      const int64_t r = row_of(off, n, j0 + k);
      if (!b64_byte_ok(off, chars, r, j0 + k)) report_row(err, valid, r);
    }
  }
  for (int64_t r = first; r < n; r += stride) {
    int64_t o = 0;
    if (valid == nullptr || valid[r]) {
      o = b64_row_outlen(chars + off[r], off[r + 1] - off[r]);
      if (o < 0) {
        atomicMin(err, (unsigned long long)r);
        o = 0;
      }
    }
    lens[r] = o;
  }
}

constexpr int kB64Tile = 128;   // rows whose offsets a block stages in LDS

// Output bytes [max(j0, lo), min(j0 + 8, hi)) of a tile: so / si are the tile's nrows + 1 output and
// input offsets, [lo, hi) = [so[0], so[nrows]) its output range, j0 a multiple of 8. A whole chunk is
// one 8-byte store (out is 8-byte aligned), a clipped one goes bytewise: its other bytes belong to
// the neighbouring tile. Every input read lies inside its own row.
template <bool kEnc>
__device__ __forceinline__ void b64_chunk(const int64_t* so, const int64_t* si, int nrows,
                                          const uint8_t* __restrict__ chars, uint8_t* __restrict__ out, int64_t j0,
                                          int64_t lo, int64_t hi) {
  const int64_t a = j0 > lo ? j0 : lo, b = j0 + 8 < hi ? j0 + 8 : hi;
  if (a >= b) return;
  int64_t r = row_of(so, nrows, a);
  uint64_t acc = 0;
  for (int64_t j = a; j < b; ++j) {
    while (so[r + 1] <= j) ++r;          // j < hi = so[nrows], so r stays below nrows
    const int64_t q = j - so[r];
    uint8_t byte;
    if (kEnc) {
      const int c = (int)(q & 3);
      const int64_t p = si[r] + 3 * (q >> 2) + c, end = si[r + 1];
      const int l = c > 0 ? chars[p - 1] : 0;
      const int h = (c < 3 && p < end) ? chars[p] : 0;
      const int v = c == 0 ? h >> 2 : c == 1 ? ((l & 3) << 4) | (h >> 4) : c == 2 ? ((l & 15) << 2) | (h >> 6) : l & 63;
      byte = b64_chr(v);
    } else {
      const int c = (int)(q % 3);
      const int64_t p = si[r] + 4 * (q / 3) + c;
      const int x = b64_val(chars[p]), y = b64_val(chars[p + 1]);
      byte = (uint8_t)(c == 0 ? ((x & 63) << 2) | ((y >> 4) & 3)
                              : c == 1 ? ((x & 15) << 4) | ((y >> 2) & 15) : ((x & 3) << 6) | (y & 63));
    }
    acc |= (uint64_t)byte << (8 * (j - j0));
  }
  if (b - a == 8) {
    *reinterpret_cast<uint64_t*>(out + j0) = acc;
  } else {
    for (int64_t j = a; j < b; ++j) out[j] = (uint8_t)(acc >> (8 * (j - j0)));
  }
}

template <bool kEnc>
__global__ __launch_bounds__(kBlock) void b64_write_kernel(const int64_t* __restrict__ ioff,
                                                         const uint8_t* __restrict__ chars,
                                                         const int64_t* __restrict__ ooff, int64_t n,
                                                         int64_t out_cap, uint8_t* __restrict__ out) {
  __shared__ int64_t so[kB64Tile + 1], si[kB64Tile + 1];
  const int64_t tiles = (n + kB64Tile - 1) / kB64Tile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kB64Tile;
    const int nr = (int)(n - r0 < kB64Tile ? n - r0 : kB64Tile);
    __syncthreads();                       // the previous tile's readers are done
    for (int i = threadIdx.x; i <= nr; i += blockDim.x) {
      so[i] = ooff[r0 + i];
      si[i] = ioff[r0 + i];
    }
    __syncthreads();
    // (clipped to the size of out: the host sized it from a readback that a replay may hand back stale)
    const int64_t lo = so[0], hi = so[nr] < out_cap ? so[nr] : out_cap;
    for (int64_t j0 = (lo & ~(int64_t)7) + 8 * (int64_t)threadIdx.x; j0 < hi; j0 += 8 * (int64_t)blockDim.x)
      b64_chunk<kEnc>(so, si, nr, chars, out, j0, lo, hi);
  }
}

// ---------------------------------------------------------------- utf-8
// One row on its own: no overlong form, surrogate, value above U+10FFFF, stray continuation byte or
// sequence cut off by the row's end.
__device__ __forceinline__ bool utf8_row_ok(const uint8_t* s, int64_t len) {
  int64_t i = 0;
  while (i < len) {
    const uint8_t c = s[i];
    if (c < 0x80) {
      ++i;
      continue;
    }
    if (c < 0xC2 || c > 0xF4) return false;           // continuation, C0 / C1 overlong, F5..FF
    const int need = c < 0xE0 ? 1 : c < 0xF0 ? 2 : 3;
    if (i + need >= len) return false;
    const uint8_t c1 = s[i + 1];
    if ((c1 & 0xC0) != 0x80) return false;
    if (c == 0xE0 && c1 < 0xA0) return false;         // overlong 3-byte
    if (c == 0xED && c1 >= 0xA0) return false;        // surrogates
    if (c == 0xF0 && c1 < 0x90) return false;         // overlong 4-byte
    if (c == 0xF4 && c1 >= 0x90) return false;        // above U+10FFFF
    for (int k = 2; k <= need; ++k)
      if ((s[i + k] & 0xC0) != 0x80) return false;
    i += need + 1;
  }
  return true;
}

// some byte of [j0, min(j0 + 16, nbytes)) has its high bit set (one lane's share of a tile)
__device__ __forceinline__ bool utf8_lane_high(const uint8_t* __restrict__ in, int64_t nbytes, int64_t j0) {
  uint64_t v[2] = {0, 0};
  if (j0 + 16 <= nbytes) {
    __builtin_memcpy(v, in + j0, 16);
  } else {
    for (int64_t j = j0; j < nbytes; ++j) v[0] |= in[j];
  }
  return ((v[0] | v[1]) & 0x8080808080808080ull) != 0;
}

// flags[t] = some byte of [t * kUtf8Tile, (t + 1) * kUtf8Tile) has its high bit set; one block per tile
__global__ __launch_bounds__(kBlock) void utf8_tile_flags_kernel(const uint8_t* __restrict__ in, int64_t nbytes,
                                                               uint8_t* __restrict__ flags) {
  const int64_t j0 = (int64_t)blockIdx.x * kUtf8Tile + 16 * (int64_t)threadIdx.x;
  const int any = __syncthreads_or(utf8_lane_high(in, nbytes, j0));
  if (threadIdx.x == 0) flags[blockIdx.x] = (uint8_t)(any != 0);
}

// tile t covers bytes [t * kUtf8Tile, ...) of chars, as the offsets count them. err[0]: smallest invalid row.
__global__ __launch_bounds__(kBlock) void utf8_validate_kernel(const int64_t* __restrict__ off,
                                                             const uint8_t* __restrict__ chars,
                                                             const uint8_t* __restrict__ valid, int64_t n,
                                                             const uint8_t* __restrict__ flags,
                                                             unsigned long long* __restrict__ err) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = off[r], e = off[r + 1];
    if (e <= b || (valid != nullptr && !valid[r])) continue;
    bool any = false;
    for (int64_t t = b / kUtf8Tile; t <= (e - 1) / kUtf8Tile && !any; ++t) any = flags[t] != 0;
    if (any && !utf8_row_ok(chars + b, e - b)) atomicMin(err, (unsigned long long)r);
  }
}

}  // namespace

void bin_hex_encode(const uint8_t* in, int64_t nbytes, uint8_t* out, hipStream_t s) {
  if (nbytes == 0) return;
  hipLaunchKernelGGL(hex_encode_kernel, dim3(grid_for(nbytes, kBlock * 8, 65536)), dim3(kBlock), 0, s, in, nbytes, out);
  check_launch("bin_hex_encode", s);
}

void bin_hex_validate(const int64_t* off, const uint8_t* chars, const uint8_t* valid, int64_t n, int64_t nbytes,
                      int64_t* err, hipStream_t s) {   // nbytes: an upper bound of off[n] - off[0], sizes the grid
  if (n == 0) return;
  const int64_t work = n > nbytes / 8 ? n : nbytes / 8;
  hipLaunchKernelGGL(hex_validate_kernel, dim3(grid_for(work, kBlock, 65536)), dim3(kBlock), 0, s, off, chars, valid, n,
                     reinterpret_cast<unsigned long long*>(err));
  check_launch("bin_hex_validate", s);
}

void bin_hex_decode(const int64_t* off, int64_t n, const uint8_t* in, int64_t nout, uint8_t* out, hipStream_t s) {
  if (n == 0 || nout == 0) return;   // nout: the size of out; the kernel writes min(nout, (off[n] - off[0]) / 2) bytes
  hipLaunchKernelGGL(hex_decode_kernel, dim3(grid_for(nout, kBlock * 8, 65536)), dim3(kBlock), 0, s, off, n, in, nout,
                     out);
  check_launch("bin_hex_decode", s);
}

void bin_b64_enc_lengths(const int64_t* off, const uint8_t* valid, int64_t n, int64_t* lens, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(b64_enc_lengths_kernel, dim3(grid_for(n, kBlock, 65536)), dim3(kBlock), 0, s, off, valid, n, lens);
  check_launch("bin_b64_enc_lengths", s);
}

void bin_b64_dec_lengths(const int64_t* off, const uint8_t* chars, const uint8_t* valid, int64_t n, int64_t nbytes,
                         int64_t* lens, int64_t* err, hipStream_t s) {
  if (n == 0) return;
  const int64_t work = n > nbytes / 8 ? n : nbytes / 8;
  hipLaunchKernelGGL(b64_dec_lengths_kernel, dim3(grid_for(work, kBlock, 65536)), dim3(kBlock), 0, s, off, chars, valid,
                     n, lens, reinterpret_cast<unsigned long long*>(err));
  check_launch("bin_b64_dec_lengths", s);
}

void bin_b64_write(bool encode, const int64_t* ioff, const uint8_t* chars, const int64_t* ooff, int64_t n,
                   int64_t out_cap, uint8_t* out, hipStream_t s) {
  if (n == 0 || out_cap <= 0) return;
  if ((reinterpret_cast<uintptr_t>(out) & 7) != 0) throw std::runtime_error("bin_b64_write: output not 8-byte aligned");
  const dim3 g(grid_for(n, kB64Tile, 1 << 20));
  if (encode) hipLaunchKernelGGL(b64_write_kernel<true>, g, dim3(kBlock), 0, s, ioff, chars, ooff, n, out_cap, out);
  else hipLaunchKernelGGL(b64_write_kernel<false>, g, dim3(kBlock), 0, s, ioff, chars, ooff, n, out_cap, out);
  check_launch("bin_b64_write", s);
}

int64_t utf8_num_tiles(int64_t nbytes) { return (nbytes + kUtf8Tile - 1) / kUtf8Tile; }

void utf8_validate(const int64_t* off, const uint8_t* chars, const uint8_t* valid, int64_t n, int64_t nbytes,
                   uint8_t* flags, int64_t* err, hipStream_t s) {
  if (n == 0 || nbytes == 0) return;
  hipLaunchKernelGGL(utf8_tile_flags_kernel, dim3((unsigned)utf8_num_tiles(nbytes)), dim3(kBlock), 0, s, chars, nbytes,
                     flags);
  check_launch("utf8_tile_flags", s);
  hipLaunchKernelGGL(utf8_validate_kernel, dim3(grid_for(n, kBlock, 65536)), dim3(kBlock), 0, s, off, chars, valid, n,
                     flags, reinterpret_cast<unsigned long long*>(err));
  check_launch("utf8_validate", s);
}

}  // namespace kern
}  // namespace igloo
