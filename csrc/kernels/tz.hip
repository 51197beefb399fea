// Time-zone conversion of int64 microsecond timestamps (TIMESTAMP WITH TIME
// ZONE): UTC -> local wall time, wall time -> UTC, date_trunc and date_part in
// the zone's local time.
//
// A zone is a flat table compiled on the host (igloo_amd/utils/tzdb.py), one
// device buffer of P = 2^k padded entries:
//   trans[P]  int64  transition instants, UTC seconds, sorted, INT64_MAX padded
//   wall[P]   int64  wall-clock switch points, trans[i] + max(off before, off after)
//   offs[P]   int32  offs[i] = UTC offset in seconds in force after i transitions
// The offset of an instant s is offs[#{trans <= s}]; that of a wall time w is
// offs[#{wall <= w}], which reads a wall time inside a gap or a fold with the
// offset in force before the transition (PEP 495 fold = 0). A zone whose POSIX
// rule repeats forever is expanded over one 400-year Gregorian cycle
// (146097 days, a whole number of weeks); later values fold back by whole
// cycles from utc_lo / wall_lo.
//
// Every workgroup copies the arrays its mode needs into LDS once, then
// grid-strides over row pairs: one 16-byte load, two upper-bound searches of
// fixed depth k without branches (all lanes run the same k steps), one
// 16-byte store (8 bytes for int32 results). The pairing starts at the first
// 16-byte boundary of the input, so a sliced column keeps aligned loads; the
// at most two rows left over are done one at a time. A fixed-offset zone
// (log2p < 0) takes an instantiation without LDS and without the search.
// NULL rows may hold any bits: all arithmetic on values wraps, the search
// index stays inside the table.
#include "civil.h"
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace igloo {
namespace kern {

namespace {

constexpr int64_t kCycleS = 146097LL * 86400LL;   // 400 Gregorian years in seconds
constexpr int64_t kUsSec = 1000000LL;
constexpr int64_t kUsDay = 86400LL * kUsSec;
constexpr int kTzMaxBlocks = 2048;                // 256 CUs x 8 workgroups

enum Mode : int { kToLocal = 0, kToUtc = 1, kTrunc = 2, kPart = 3 };

typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
typedef int32_t i32x2 __attribute__((ext_vector_type(2)));

__device__ inline int64_t floor_div(int64_t a, int64_t b) {   // b > 1
  const int64_t q = a / b;
  return q - ((a - q * b) < 0 ? 1 : 0);
}
__device__ inline int64_t wrap_add(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
__device__ inline int64_t wrap_mul(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b); }

template <bool Fixed>
struct Zone {
  const int64_t* trans;
  const int64_t* wall;
  const int32_t* offs;
  int p;                 // padded entry count, a power of two
  int fixed;             // the offset of a fixed-offset zone
  int64_t utc_lo, wall_lo;

  __device__ inline int search(const int64_t* keys, int64_t lo, int64_t s) const {
    s = s >= lo + kCycleS ? lo + (s - lo) % kCycleS : s;
    int pos = 0;
    for (int h = p >> 1; h > 0; h >>= 1) pos += keys[pos + h - 1] <= s ? h : 0;   // pos < p: the last key is padding
    return offs[pos];
  }
  __device__ inline int off_utc(int64_t us) const {
    if (Fixed) return fixed;
    return search(trans, utc_lo, floor_div(us, kUsSec));
  }
  __device__ inline int off_wall(int64_t us) const {
    if (Fixed) return fixed;
    return search(wall, wall_lo, floor_div(us, kUsSec));
  }
};

__device__ inline int64_t trunc_local(int64_t l, int unit) {
  if (unit <= 2) {
    const int64_t step = unit == 0 ? kUsSec : unit == 1 ? 60 * kUsSec : 3600 * kUsSec;
    return wrap_mul(floor_div(l, step), step);
  }
  int64_t days = floor_div(l, kUsDay);
  if (unit == 4) {   // week: back to Monday (1970-01-01 was a Thursday)
    int64_t wd = (days + 3) % 7;
    days -= wd < 0 ? wd + 7 : wd;
  } else if (unit >= 5) {
    int y, m, d;
    civil(days, &y, &m, &d);
    if (unit == 6) m = (m - 1) / 3 * 3 + 1;
    if (unit == 7) m = 1;
    days = days_from_civil(y, m, 1);
  }
  return wrap_mul(days, kUsDay);
}

// field codes: 0..5 as date_part (year month day quarter dow doy), then hour
// minute second millisecond microsecond week (the naive ts_part's values)
__device__ inline int32_t part_local(int64_t l, int field) {
  const int64_t days = floor_div(l, kUsDay);
  const int64_t rem = l - days * kUsDay;
  switch (field) {
    case 6: return (int32_t)(rem / (3600 * kUsSec));
    case 7: return (int32_t)(rem / (60 * kUsSec) % 60);
    case 8: return (int32_t)(rem / kUsSec % 60);
    case 9: return (int32_t)(rem / 1000 % 60000);
    case 10: return (int32_t)(rem % (60 * kUsSec));
    default: break;
  }
  if (field == 4) {
    const int64_t r = (days + 4) % 7;
    return (int32_t)(r < 0 ? r + 7 : r);
  }
  int y, m, d;
  if (field == 11) {   // ISO week: the week of this row's Thursday
    int64_t wd = (days + 3) % 7;
    wd = wd < 0 ? wd + 7 : wd;
    const int64_t thu = days - wd + 3;
    civil(thu, &y, &m, &d);
    return (int32_t)((thu - days_from_civil(y, 1, 1)) / 7 + 1);
  }
  civil(days, &y, &m, &d);
  switch (field) {
    case 0: return y;
    case 1: return m;
    case 2: return d;
    case 3: return (m - 1) / 3 + 1;
    default: return (int32_t)(days - days_from_civil(y, 1, 1) + 1);
  }
}

template <int M> struct out_of { using type = int64_t; using vec = i64x2; };
template <> struct out_of<kPart> { using type = int32_t; using vec = i32x2; };

template <int M, bool Fixed>
__device__ inline typename out_of<M>::type row(const Zone<Fixed>& z, int64_t v, int arg, int* off) {
  if (M == kToUtc) return wrap_add(v, -wrap_mul(z.off_wall(v), kUsSec));
  *off = z.off_utc(v);
  const int64_t l = wrap_add(v, wrap_mul(*off, kUsSec));
  if (M == kToLocal) return l;
  if (M == kPart) return part_local(l, arg);
  const int64_t t = trunc_local(l, arg);
  return wrap_add(t, -wrap_mul(z.off_wall(t), kUsSec));
}

template <int M, bool Fixed>
__global__ __launch_bounds__(kBlock) void tz_kernel(const int64_t* __restrict__ in, int64_t n,
                                                   const int64_t* __restrict__ tab, int p, int fixed, int64_t utc_lo,
                                                   int64_t wall_lo, int arg, typename out_of<M>::type* __restrict__ out,
                                                   int32_t* __restrict__ off_out) {
  using O = typename out_of<M>::type;
  using OV = typename out_of<M>::vec;
  extern __shared__ __align__(16) unsigned char tz_lds[];
  Zone<Fixed> z;
  z.p = p;
  z.fixed = fixed;
  z.utc_lo = utc_lo;
  z.wall_lo = wall_lo;
  if (!Fixed) {
    // LDS: [trans][wall][offs], each only if this mode searches it
    constexpr bool kUtcKeys = M != kToUtc, kWallKeys = M == kToUtc || M == kTrunc;
    int64_t* lt = reinterpret_cast<int64_t*>(tz_lds);
    int64_t* lw = lt + (kUtcKeys ? p : 0);
    int32_t* lo = reinterpret_cast<int32_t*>(lw + (kWallKeys ? p : 0));
    const int32_t* goffs = reinterpret_cast<const int32_t*>(tab + 2 * (int64_t)p);
    for (int i = threadIdx.x; i < p; i += blockDim.x) {
      if (kUtcKeys) lt[i] = tab[i];
      if (kWallKeys) lw[i] = tab[p + i];
      lo[i] = goffs[i];
    }
    z.trans = lt;
    z.wall = lw;
    z.offs = lo;
    __syncthreads();
  }
  const int head = (int)((reinterpret_cast<uintptr_t>(in) >> 3) & 1);   // n >= 1: checked by the launcher
  const int64_t pairs = (n - head) / 2;
  const bool vec_store = (((reinterpret_cast<uintptr_t>(out) / sizeof(O)) + head) & 1) == 0;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < pairs; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = head + 2 * q;
    const i64x2 v = *reinterpret_cast<const i64x2*>(in + r);
    int o0 = 0, o1 = 0;
    OV w;
    w.x = row<M, Fixed>(z, v.x, arg, &o0);
    w.y = row<M, Fixed>(z, v.y, arg, &o1);
    if (vec_store) {
      *reinterpret_cast<OV*>(out + r) = w;
    } else {
      out[r] = w.x;
      out[r + 1] = w.y;
    }
    if (M == kToLocal && off_out) {
      off_out[r] = o0;
      off_out[r + 1] = o1;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) {   // the row before the first pair, the row after the last
    int64_t r = -1;
    if (threadIdx.x == 0 && head) r = 0;
    if (threadIdx.x == 1 && ((n - head) & 1)) r = n - 1;
    if (r >= 0) {
      int o = 0;
      out[r] = row<M, Fixed>(z, in[r], arg, &o);
      if (M == kToLocal && off_out) off_out[r] = o;
    }
  }
}

template <int M>
void tz_launch(const char* what, const int64_t* in, int64_t n, const int64_t* tab, int log2p, int fixed,
               int64_t utc_lo, int64_t wall_lo, int arg, typename out_of<M>::type* out, int32_t* off_out,
               hipStream_t s) {
  if (n <= 0) return;
  // 2048 entries: tz_trunc stages 20 bytes per entry, 40 KiB, inside the 64 KiB of dynamic LDS a launch
  // gets without raising the function's limit (utils/tzdb.py refuses larger zones when it compiles them)
  if (log2p > 11) throw std::runtime_error(std::string(what) + ": zone table larger than 2048 entries");
  const int p = log2p < 0 ? 0 : 1 << log2p;
  const size_t lds = (size_t)p * ((M == kTrunc ? 16 : 8) + 4);
  const dim3 g(grid_for((n + 1) / 2, kBlock, kTzMaxBlocks)), b(kBlock);
  dispatch(log2p < 0, [&](auto f) {
    launch(what, tz_kernel<M, f.value>, g, b, f.value ? 0 : lds, s, in, n, tab, p, fixed, utc_lo, wall_lo, arg, out,
           off_out);
  });
}

}  // namespace

void tz_to_local(const int64_t* in, int64_t n, const int64_t* tab, int log2p, int fixed_off, int64_t utc_lo,
                 int64_t wall_lo, int64_t* out, int32_t* off_out, hipStream_t s) {
  tz_launch<kToLocal>("tz_to_local", in, n, tab, log2p, fixed_off, utc_lo, wall_lo, 0, out, off_out, s);
}

void tz_to_utc(const int64_t* in, int64_t n, const int64_t* tab, int log2p, int fixed_off, int64_t utc_lo,
               int64_t wall_lo, int64_t* out, hipStream_t s) {
  tz_launch<kToUtc>("tz_to_utc", in, n, tab, log2p, fixed_off, utc_lo, wall_lo, 0, out, nullptr, s);
}

void tz_trunc(const int64_t* in, int64_t n, const int64_t* tab, int log2p, int fixed_off, int64_t utc_lo,
              int64_t wall_lo, int unit, int64_t* out, hipStream_t s) {
  if (unit < 0 || unit > 7) throw std::runtime_error("tz_trunc: unknown unit");
  tz_launch<kTrunc>("tz_trunc", in, n, tab, log2p, fixed_off, utc_lo, wall_lo, unit, out, nullptr, s);
}

void tz_part(const int64_t* in, int64_t n, const int64_t* tab, int log2p, int fixed_off, int64_t utc_lo,
             int64_t wall_lo, int field, int32_t* out, hipStream_t s) {
  if (field < 0 || field > 11) throw std::runtime_error("tz_part: unknown field");
  tz_launch<kPart>("tz_part", in, n, tab, log2p, fixed_off, utc_lo, wall_lo, field, out, nullptr, s);
}

}  // namespace kern
}  // namespace igloo
