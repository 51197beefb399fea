// Checked numeric conversion, one value at a time: the element routines of
// the cast_checked kernel (trycast.hip). Every routine returns false where
// TRY_CAST gives NULL and otherwise writes exactly the value plain CAST gives.
// __host__ __device__ and free of device intrinsics, so the same code compiles
// into the stand-alone sanitizer driver (csrc/tools/trycast_host.cpp).
//
// Range decisions are made in integers, or in doubles that are exact: the
// bounds of a b-bit integer target are -2^(b-1) (inclusive) and 2^(b-1)
// (exclusive), both powers of two. (double)INT64_MAX would round up to 2^63
// and is never used.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IGLOO_HD __host__ __device__
#else
#define IGLOO_HD
#endif

namespace igloo {
namespace kern {

// source / destination kinds of cast_checked (the Python side passes these numbers)
enum CastKind : int {
  kCastI8 = 0,
  kCastI16 = 1,
  kCastI32 = 2,
  kCastI64 = 3,
  kCastF32 = 4,
  kCastF64 = 5,
  kCastDec = 6,    // int64 fixed point at a scale
  kCastWide = 7,   // int128 fixed point: (low, high) int64 words per row; source only
};

// tags for the two sources that are not told apart by their storage type
struct dec_src { int64_t v; };
struct wide_src { int64_t lo, hi; };

// Everything that depends on the (source, target) scales only, worked out once per launch.
struct CastPlan {
  int32_t up;          // target scale - source scale
  int32_t precision;   // of a decimal target; > 18: no bound beyond int64
  int64_t mul;         // 10^up for 0 <= up <= 18, else 0 (only 0 survives such a rescale)
  uint64_t div;        // 10^-up for -19 <= up < 0 (rescale), 10^source scale for an integer target; 0: above 10^19
  uint64_t wdiv_lo;    // the same divisor as 128 bits, up to 10^38 (wide sources)
  uint64_t wdiv_hi;
  int64_t bound;       // 10^precision for precision <= 18, else 0
  double fmul;         // 10^target scale, the factor CAST multiplies a float by
};

IGLOO_HD inline unsigned __int128 cast_pow10_u128(int e) {
  unsigned __int128 v = 1;
  for (int k = 0; k < e; ++k) v *= 10;
  return v;
}

// dst_is_decimal == false: an integer target (only src_scale matters)
IGLOO_HD inline CastPlan make_cast_plan(int src_scale, bool dst_is_decimal, int dst_scale, int dst_precision) {
  CastPlan p;
  p.up = dst_is_decimal ? dst_scale - src_scale : -src_scale;
  p.precision = dst_precision;
  p.mul = (p.up >= 0 && p.up <= 18) ? (int64_t)cast_pow10_u128(p.up) : 0;
  const int down = p.up < 0 ? -p.up : 0;
  p.div = down <= 19 ? (uint64_t)cast_pow10_u128(down) : 0;
  const unsigned __int128 w = cast_pow10_u128(down <= 38 ? down : 38);
  p.wdiv_lo = (uint64_t)w;
  p.wdiv_hi = (uint64_t)(w >> 64);
  p.bound = (dst_is_decimal && dst_precision <= 18) ? (int64_t)cast_pow10_u128(dst_precision) : 0;
  double f = 1.0;
  for (int k = 0; k < dst_scale; ++k) f *= 10.0;   // exact up to 10^22, as the host's float(10**s)
  p.fmul = dst_is_decimal ? f : 1.0;
  return p;
}

template <typename D> struct int_bounds;
template <> struct int_bounds<int8_t> { static constexpr int64_t lo = -128, hi = 127; static constexpr double pow2 = 0x1p7; };
template <> struct int_bounds<int16_t> { static constexpr int64_t lo = -32768, hi = 32767; static constexpr double pow2 = 0x1p15; };
template <> struct int_bounds<int32_t> { static constexpr int64_t lo = -2147483648LL, hi = 2147483647LL; static constexpr double pow2 = 0x1p31; };
template <> struct int_bounds<int64_t> { static constexpr int64_t lo = INT64_MIN, hi = INT64_MAX; static constexpr double pow2 = 0x1p63; };

template <typename D> IGLOO_HD inline bool fit_int(int64_t v, D* out) {
  if (v < int_bounds<D>::lo || v > int_bounds<D>::hi) return false;
  *out = (D)v;
  return true;
}

IGLOO_HD inline __int128 wide_value(wide_src w) {
  return (__int128)(((unsigned __int128)(uint64_t)w.hi << 64) | (uint64_t)w.lo);
}

IGLOO_HD inline bool fit_i64(__int128 v, int64_t* out) {
  if (v > (__int128)INT64_MAX || v < (__int128)INT64_MIN) return false;
  *out = (int64_t)v;
  return true;
}

// |v| < 10^precision for a decimal target of at most 18 digits
IGLOO_HD inline bool fit_precision(int64_t v, const CastPlan& p) {
  return p.bound == 0 || (v > -p.bound && v < p.bound);
}

// truncating division of an int64 by 10^k (p.div; 0 stands for a divisor above 10^19 > |v|)
IGLOO_HD inline int64_t trunc_div(int64_t v, uint64_t div) {
  if (div == 0) return 0;
  const uint64_t u = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
  const uint64_t q = u / div;               // q <= 2^63, and 2^63 only for v == INT64_MIN, div == 1
  return v < 0 ? (int64_t)((uint64_t)0 - q) : (int64_t)q;
}

// ---- to an integer target ---------------------------------------------------
template <typename D, typename S> IGLOO_HD inline bool cast_to_int(S v, const CastPlan&, D* out) {
  return fit_int<D>((int64_t)v, out);                      // int8 .. int64 sources
}
template <typename D> IGLOO_HD inline bool cast_to_int(double x, const CastPlan&, D* out) {
  const double t = __builtin_trunc(x);                     // toward zero, as CAST; NaN fails both comparisons
  if (!(t >= -int_bounds<D>::pow2 && t < int_bounds<D>::pow2)) return false;
  *out = (D)(int64_t)t;
  return true;
}
template <typename D> IGLOO_HD inline bool cast_to_int(float x, const CastPlan& p, D* out) {
  return cast_to_int<D>((double)x, p, out);                // every float is a double
}
template <typename D> IGLOO_HD inline bool cast_to_int(dec_src s, const CastPlan& p, D* out) {
  return fit_int<D>(trunc_div(s.v, p.div), out);
}
template <typename D> IGLOO_HD inline bool cast_to_int(wide_src s, const CastPlan& p, D* out) {
  const __int128 v = wide_value(s);
  const unsigned __int128 div = ((unsigned __int128)p.wdiv_hi << 64) | p.wdiv_lo;
  __int128 q = v;
  if (div != 1) {
    const unsigned __int128 u = v < 0 ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    const unsigned __int128 uq = u / div;                  // < 2^127 / 10
    q = v < 0 ? -(__int128)uq : (__int128)uq;
  }
  int64_t r;
  return fit_i64(q, &r) && fit_int<D>(r, out);
}

// ---- to a decimal target (int64 at the target scale) --------------------------
// an int64 value at the source scale, rescaled: up: exact product; down: round half away from zero
IGLOO_HD inline bool rescale_i64(int64_t v, const CastPlan& p, int64_t* out) {
  int64_t r;
  if (p.up >= 0) {
    if (p.mul == 0) {
      if (v != 0) return false;                            // |v| * 10^19 and up never fits
      r = 0;
    } else if (!fit_i64((__int128)v * p.mul, &r)) {
      return false;
    }
  } else if (p.div == 0) {
    r = 0;                                                 // |v| < 2^63 < 10^20 / 2
  } else {
    const uint64_t u = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
    const uint64_t q = (u + p.div / 2) / p.div;            // u <= 2^63, div / 2 <= 5 * 10^18: no wrap; q < 2^63
    r = v < 0 ? -(int64_t)q : (int64_t)q;
  }
  if (!fit_precision(r, p)) return false;
  *out = r;
  return true;
}
template <typename S> IGLOO_HD inline bool cast_to_dec(S v, const CastPlan& p, int64_t* out) {
  return rescale_i64((int64_t)v, p, out);
}
IGLOO_HD inline bool cast_to_dec(dec_src s, const CastPlan& p, int64_t* out) { return rescale_i64(s.v, p, out); }
IGLOO_HD inline bool cast_to_dec(wide_src s, const CastPlan& p, int64_t* out) {
  const __int128 v = wide_value(s);
  int64_t r;
  if (p.up >= 0) return fit_i64(v, &r) && rescale_i64(r, p, out);
  const unsigned __int128 div = ((unsigned __int128)p.wdiv_hi << 64) | p.wdiv_lo;
  const unsigned __int128 u = v < 0 ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
  const unsigned __int128 q = (u + div / 2) / div;         // u <= 2^127, div / 2 <= 5 * 10^37: below 2^128
  if (q > (unsigned __int128)INT64_MAX + (v < 0 ? 1 : 0)) return false;
  r = v < 0 ? (int64_t)((uint64_t)0 - (uint64_t)q) : (int64_t)(uint64_t)q;
  if (!fit_precision(r, p)) return false;
  *out = r;
  return true;
}
// rint(x * 10^s), half to even; the product is formed in the source's own precision, as CAST forms it
IGLOO_HD inline bool cast_to_dec(double x, const CastPlan& p, int64_t* out) {
  const double t = __builtin_rint(x * p.fmul);
  if (!(t >= -0x1p63 && t < 0x1p63)) return false;
  const int64_t r = (int64_t)t;
  if (!fit_precision(r, p)) return false;
  *out = r;
  return true;
}
IGLOO_HD inline bool cast_to_dec(float x, const CastPlan& p, int64_t* out) {
  const float t = __builtin_rintf(x * (float)p.fmul);
  if (!(t >= -0x1p63f && t < 0x1p63f)) return false;
  const int64_t r = (int64_t)t;
  if (!fit_precision(r, p)) return false;
  *out = r;
  return true;
}

}  // namespace kern
}  // namespace igloo
