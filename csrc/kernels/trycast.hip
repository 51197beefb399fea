// TRY_CAST kernels (gfx950): conversions that write a validity byte per row
// in place of raising, so neither needs an error flag or a readback and both
// can be captured in a query graph.
//
//   try_parse     varchar -> int8/16/32/64, decimal(p, s), float64, float32,
//                 date, bool, timestamp. One lane per row over the Arrow
//                 large-string layout, as str_parse (strexpr.hip), through the
//                 same device routines of textparse.h; the integer range is
//                 checked here, at the target's own width.
//   cast_checked  int8/16/32/64, float32/64, decimal (int64) and wide (int128)
//                 -> int8/16/32/64 or decimal(p, s), NULL where the value does
//                 not fit (castcheck.h). Pure streaming: each lane owns 8
//                 consecutive rows, moves them as 16-byte vectors where the
//                 pointers allow and writes their 8 validity bytes as one
//                 8-byte store.
//
// Alignment is a property of the call, not an assumption: a tensor view starts
// at any element. cast_checked converts the first `head` rows one by one so
// that the source is vector aligned from there on, then decides per array
// (source, target, both validity arrays) whether row head + 8k sits on a
// vector boundary; an array that does not takes element accesses. All of these
// decisions are the same for every lane of the launch.
#include "castcheck.h"
#include "common.h"
#include "kernels.h"
#include "launch.h"
#include "textparse.h"

namespace igloo {
namespace kern {

namespace {

// ---------------------------------------------------------------- try_parse
// kind: 0 int64, 1 int32, 2 decimal -> int64 at `scale` (|v| < 10^precision for precision <= 18),
// 3 date32, 4 float64, 5 bool, 6 int16, 7 int8, 8 float32, 9 timestamp (int64 microseconds)
__global__ __launch_bounds__(kBlock) void try_parse_kernel(const int64_t* __restrict__ off,
                                                           const uint8_t* __restrict__ chars, int64_t n,
                                                           const uint8_t* __restrict__ valid, int kind, int scale,
                                                           int64_t bound, void* __restrict__ out,
                                                           uint8_t* __restrict__ valid_out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    // absolute offsets: a sliced column starts at off[0] > 0 in the parent's bytes
    const uint8_t* p = chars + off[i];
    const uint8_t* e = chars + off[i + 1];
    bool ok = !(valid && !valid[i]);
    switch (kind) {
      case 0:
      case 1:
      case 6:
      case 7: {
        int64_t v = 0;
        ok = ok && parse_int(p, e, &v);
        if (kind == 0) {
          static_cast<int64_t*>(out)[i] = ok ? v : 0;
        } else if (kind == 1) {
          ok = ok && v >= INT32_MIN && v <= INT32_MAX;
          static_cast<int32_t*>(out)[i] = ok ? (int32_t)v : 0;
        } else if (kind == 6) {
          ok = ok && v >= INT16_MIN && v <= INT16_MAX;
          static_cast<int16_t*>(out)[i] = ok ? (int16_t)v : 0;
        } else {
          ok = ok && v >= INT8_MIN && v <= INT8_MAX;
          static_cast<int8_t*>(out)[i] = ok ? (int8_t)v : 0;
        }
        break;
      }
      case 2: {
        int64_t v = 0;
        ok = ok && parse_decimal(p, e, scale, &v);
        ok = ok && (bound == 0 || (v > -bound && v < bound));
        static_cast<int64_t*>(out)[i] = ok ? v : 0;
        break;
      }
      case 3: {
        int32_t v = 0;
        ok = ok && parse_date(p, e, &v);
        static_cast<int32_t*>(out)[i] = ok ? v : 0;
        break;
      }
      case 4:
      case 8: {
        double v = 0;
        ok = ok && parse_f64(p, e, &v);
        if (kind == 4) static_cast<double*>(out)[i] = ok ? v : 0.0;
        else static_cast<float*>(out)[i] = ok ? (float)v : 0.0f;   // the correctly rounded double, rounded once more
        break;
      }
      case 5: {
        uint8_t v = 0;
        if (ok) {
          if (ieq(p, e, "true") || ieq(p, e, "t") || ieq(p, e, "1")) v = 1;
          else ok = ieq(p, e, "false") || ieq(p, e, "f") || ieq(p, e, "0");
        }
        static_cast<uint8_t*>(out)[i] = v;
        break;
      }
      default: {
        int64_t v = 0;
        ok = ok && parse_timestamp(p, e, &v);
        static_cast<int64_t*>(out)[i] = ok ? v : 0;
      }
    }
    valid_out[i] = ok;
  }
}

// -------------------------------------------------------------- cast_checked
constexpr int kRowsPerLane = 8;

// storage of one source row, and the value handed to castcheck.h
template <typename S> struct src_of { using store = S; static __device__ S get(S v) { return v; } };
template <> struct src_of<dec_src> { using store = int64_t; static __device__ dec_src get(int64_t v) { return dec_src{v}; } };
struct wide_words { int64_t lo, hi; };
template <> struct src_of<wide_src> {
  using store = wide_words;
  static __device__ wide_src get(wide_words w) { return wide_src{w.lo, w.hi}; }
};

struct dec_dst {};   // int64 at the target scale, against an integer target of the same storage
template <typename D> struct dst_of { using store = D; };
template <> struct dst_of<dec_dst> { using store = int64_t; };

template <typename S, typename D>
__device__ inline bool convert_one(typename src_of<S>::store s, const CastPlan& plan, typename dst_of<D>::store* out) {
  if constexpr (std::is_same<D, dec_dst>::value) return cast_to_dec(src_of<S>::get(s), plan, out);
  else return cast_to_int<D>(src_of<S>::get(s), plan, out);
}

// 8 consecutive elements between memory and registers: 16-byte (8-byte for one-byte elements)
// vector accesses when `vec`, element accesses otherwise
template <typename T> __device__ inline void load8(const T* __restrict__ p, bool vec, T (&r)[kRowsPerLane]) {
  constexpr int kBytes = kRowsPerLane * (int)sizeof(T);
  if (vec) {
    if constexpr (kBytes == 8) {
      const uint64_t w = *reinterpret_cast<const uint64_t*>(p);
      __builtin_memcpy(r, &w, 8);
    } else {
      uint4 w[kBytes / 16];
#pragma unroll
      for (int k = 0; k < kBytes / 16; ++k) w[k] = reinterpret_cast<const uint4*>(p)[k];
      __builtin_memcpy(r, w, kBytes);
    }
  } else {
#pragma unroll
    for (int k = 0; k < kRowsPerLane; ++k) r[k] = p[k];
  }
}

template <typename T> __device__ inline void store8(T* __restrict__ p, bool vec, const T (&r)[kRowsPerLane]) {
  constexpr int kBytes = kRowsPerLane * (int)sizeof(T);
  if (vec) {
    if constexpr (kBytes == 8) {
      uint64_t w;
      __builtin_memcpy(&w, r, 8);
      *reinterpret_cast<uint64_t*>(p) = w;
    } else {
      uint4 w[kBytes / 16];
      __builtin_memcpy(w, r, kBytes);
#pragma unroll
      for (int k = 0; k < kBytes / 16; ++k) reinterpret_cast<uint4*>(p)[k] = w[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < kRowsPerLane; ++k) p[k] = r[k];
  }
}

struct CastAlign {
  int64_t head;                 // leading rows converted one by one
  bool src, dst, vin, vout;     // vector accesses from row `head` on
};

template <typename S, typename D>
__global__ __launch_bounds__(kBlock) void cast_checked_kernel(const typename src_of<S>::store* __restrict__ src,
                                                              int64_t n, const uint8_t* __restrict__ valid_in,
                                                              CastPlan plan, CastAlign al,
                                                              typename dst_of<D>::store* __restrict__ dst,
                                                              uint8_t* __restrict__ valid_out) {
  using SS = typename src_of<S>::store;
  using DS = typename dst_of<D>::store;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  // rows [0, head) and the last (n - head) % 8 rows: one row per lane
  const int64_t full = (n - al.head) / kRowsPerLane;
  const int64_t tail0 = al.head + full * kRowsPerLane;
  const int64_t loose = al.head + (n - tail0);
  for (int64_t j = tid; j < loose; j += nthreads) {
    const int64_t i = j < al.head ? j : tail0 + (j - al.head);
    DS v = 0;
    bool ok = !(valid_in && !valid_in[i]);
    ok = ok && convert_one<S, D>(src[i], plan, &v);
    dst[i] = ok ? v : (DS)0;
    valid_out[i] = ok;
  }
  for (int64_t g = tid; g < full; g += nthreads) {
    const int64_t i = al.head + g * kRowsPerLane;
    SS s[kRowsPerLane];
    DS d[kRowsPerLane];
    uint8_t vi[kRowsPerLane], vo[kRowsPerLane];
    load8(src + i, al.src, s);
    if (valid_in) load8(valid_in + i, al.vin, vi);
#pragma unroll
    for (int k = 0; k < kRowsPerLane; ++k) {
      DS v = 0;
      bool ok = !(valid_in && !vi[k]);
      ok = ok && convert_one<S, D>(s[k], plan, &v);
      d[k] = ok ? v : (DS)0;
      vo[k] = ok;
    }
    store8(dst + i, al.dst, d);
    store8(valid_out + i, al.vout, vo);
  }
}

inline bool aligned_at(const void* base, int64_t byte_off, int align) {
  return ((reinterpret_cast<uintptr_t>(base) + (uintptr_t)byte_off) & (uintptr_t)(align - 1)) == 0;
}

template <typename T> constexpr int vec_align() { return kRowsPerLane * sizeof(T) == 8 ? 8 : 16; }

template <typename S, typename D>
CastAlign cast_alignment(const void* src, int64_t n, const uint8_t* valid_in, const void* dst,
                         const uint8_t* valid_out) {
  using SS = typename src_of<S>::store;
  using DS = typename dst_of<D>::store;
  constexpr int sa = vec_align<SS>();
  CastAlign al{};
  // rows until the source reaches a vector boundary (never, when it is not even element aligned,
  // or for 16-byte rows that start 8 bytes off)
  const uintptr_t mis = reinterpret_cast<uintptr_t>(src) & (uintptr_t)(sa - 1);
  const uintptr_t gap = (sa - mis) & (uintptr_t)(sa - 1);
  al.head = gap % sizeof(SS) == 0 ? (int64_t)(gap / sizeof(SS)) : 0;
  if (al.head > n) al.head = n;
  al.src = aligned_at(src, al.head * (int64_t)sizeof(SS), sa);
  al.dst = aligned_at(dst, al.head * (int64_t)sizeof(DS), vec_align<DS>());
  al.vin = valid_in != nullptr && aligned_at(valid_in, al.head, 8);
  al.vout = aligned_at(valid_out, al.head, 8);
  return al;
}

// launch-time tags: the source and target kinds become template arguments once (launch.h)
struct src_kind { int k; };
struct dst_kind { int k; };

template <typename F> void pick(src_kind s, F&& f) {
  switch (s.k) {
    case kCastI8: return f(tag<int8_t>{});
    case kCastI16: return f(tag<int16_t>{});
    case kCastI32: return f(tag<int32_t>{});
    case kCastI64: return f(tag<int64_t>{});
    case kCastF32: return f(tag<float>{});
    case kCastF64: return f(tag<double>{});
    case kCastDec: return f(tag<dec_src>{});
    case kCastWide: return f(tag<wide_src>{});
    default: throw std::runtime_error("cast_checked: unknown source kind " + std::to_string(s.k));
  }
}

template <typename F> void pick(dst_kind d, F&& f) {
  switch (d.k) {
    case kCastI8: return f(tag<int8_t>{});
    case kCastI16: return f(tag<int16_t>{});
    case kCastI32: return f(tag<int32_t>{});
    case kCastI64: return f(tag<int64_t>{});
    case kCastDec: return f(tag<dec_dst>{});
    default: throw std::runtime_error("cast_checked: unknown target kind " + std::to_string(d.k));
  }
}

}  // namespace

void try_parse(const int64_t* off, const uint8_t* chars, int64_t n, const uint8_t* valid, int kind, int scale,
               int precision, void* out, uint8_t* valid_out, hipStream_t stream) {
  if (n == 0) return;
  if (kind < 0 || kind > 9) throw std::runtime_error("try_parse: unknown kind " + std::to_string(kind));
  const int64_t bound = (kind == 2 && precision <= 18) ? (int64_t)cast_pow10_u128(precision) : 0;
  launch("try_parse", try_parse_kernel, dim3(grid_for(n, kBlock, 65536)), dim3(kBlock), 0, stream, off, chars, n,
         valid, kind, scale, bound, out, valid_out);
}

void cast_checked(const void* src, int src_kind_, int src_scale, int64_t n, const uint8_t* valid_in, int dst_kind_,
                  int dst_scale, int dst_precision, void* dst, uint8_t* valid_out, hipStream_t stream) {
  if (n == 0) return;
  const CastPlan plan = make_cast_plan(src_scale, dst_kind_ == kCastDec, dst_scale, dst_precision);
  dispatch(src_kind{src_kind_}, dst_kind{dst_kind_}, [&](auto s, auto d) {
    using S = type_of<decltype(s)>;
    using D = type_of<decltype(d)>;
    const CastAlign al = cast_alignment<S, D>(src, n, valid_in, dst, valid_out);
    const int64_t lanes = (n - al.head) / kRowsPerLane + kRowsPerLane + 16;   // 8-row groups + the loose rows
    launch("cast_checked", cast_checked_kernel<S, D>, dim3(grid_for(lanes, kBlock, 8192)), dim3(kBlock), 0, stream,
           as<typename src_of<S>::store>(src), n, valid_in, plan, al, as<typename dst_of<D>::store>(dst), valid_out);
  });
}

}  // namespace kern
}  // namespace igloo
