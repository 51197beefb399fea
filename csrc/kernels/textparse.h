// Device text <-> value helpers shared by the CSV parser (csv.hip) and the
// string expression kernels (strexpr.hip): exact integer / fixed-point /
// date parsing, float parsing, and the inverse formatting used by
// CAST(... AS VARCHAR).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "pow5_table.h"

namespace igloo {
namespace kern {

__device__ inline int64_t days_from_civil(int64_t y, int64_t m, int64_t d) {
  y -= m <= 2;
  const int64_t era = (y >= 0 ? y : y - 399) / 400;
  const int64_t yoe = y - era * 400;
  const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}

__device__ inline bool parse_int(const uint8_t* p, const uint8_t* e, int64_t* out) {
  bool neg = false;
  if (p < e && (*p == '-' || *p == '+')) neg = *p++ == '-';
  if (p >= e) return false;
  uint64_t v = 0;
  for (; p < e; ++p) {
    const unsigned d = (unsigned)*p - '0';
    if (d > 9) return false;
    if (v > (uint64_t)922337203685477580ULL || (v == 922337203685477580ULL && d > 7 + (unsigned)neg)) return false;
    v = v * 10 + d;
  }
  *out = neg ? (int64_t)(0 - v) : (int64_t)v;
  return true;
}

// exact fixed point: digits[.digits] scaled to `scale` fractional digits; at
// least one digit, leading zeros free, at most 36 significant digits
__device__ inline bool parse_decimal(const uint8_t* p, const uint8_t* e, int scale, int64_t* out) {
  bool neg = false;
  if (p < e && (*p == '-' || *p == '+')) neg = *p++ == '-';
  if (p >= e) return false;
  __int128 v = 0;
  int frac = -1, digits = 0;
  bool any = false;
  for (; p < e; ++p) {
    if (*p == '.') {
      if (frac >= 0) return false;
      frac = 0;
      continue;
    }
    const unsigned d = (unsigned)*p - '0';
    if (d > 9) return false;
    any = true;
    if (frac >= 0) {
      if (frac == scale) {
        if (d != 0) return false;  // more fractional digits than the scale: not exact
        continue;
      }
      ++frac;
    }
    v = v * 10 + d;
    if (v != 0 && ++digits > 36) return false;
  }
  if (!any) return false;
  for (int f = frac < 0 ? 0 : frac; f < scale; ++f) {
    if (v > (__int128)INT64_MAX) return false;   // out of range already: never wraps
    v *= 10;
  }
  if (neg) v = -v;
  if (v > (__int128)INT64_MAX || v < (__int128)INT64_MIN) return false;
  *out = (int64_t)v;
  return true;
}

__device__ inline bool ieq(const uint8_t* p, const uint8_t* e, const char* lit) {
  int k = 0;
  for (; p + k < e; ++k) {
    if (!lit[k]) return false;
    uint8_t c = p[k];
    if (c >= 'A' && c <= 'Z') c += 32;
    if (c != (uint8_t)lit[k]) return false;
  }
  return lit[k] == 0;
}

// ---- float64 parsing, correctly rounded (round half to even) for every input.
//
//   fast path   at most 19 digits, all of them kept, w < 2^53 and |e10| <= 22:
//               w and 10^|e10| are exact doubles, so one multiply or divide
//               rounds once (Clinger).
//   slow path   integer only, so host and device agree bit for bit. The value
//               is w * 10^q (w: the first 19 significant digits). With the
//               truncated 128-bit power T of kPow5, 5^q = (T + d) * 2^k with
//               0 <= d < 1, so the exact 192-bit product P = w' * T (w' = w
//               normalised to 64 bits) brackets the value: P <= V < P + 2^64
//               in units of the product's low end (V == P where T is exact).
//               When digits were dropped, the upper bound is taken from w + 1.
//               Both ends are rounded to a double; rounding is monotonic, so
//               when they agree that double is the answer.
//   exact path  when the ends round differently (the value is within about
//               2^-127 of a rounding boundary, or 2^-59 with dropped digits:
//               ties, and every 60th or so long input), the digits themselves
//               (up to kBigDigits of them plus a sticky flag; no boundary
//               between doubles has more than 768 significant digits) are
//               compared as a big integer with the midpoint above each
//               candidate. Never taken on shortest round-trip or %.17e text.
constexpr uint64_t kF64Inf = 0x7FF0000000000000ULL;
constexpr uint64_t kF64NaN = 0x7FF8000000000000ULL;

// (a2:a1:a0) * 2^(e - 191) with bit 63 of a2 set, i.e. a value in [2^e, 2^(e+1)),
// to the bits of the nearest double (ties to even); a1 and a0 are sticky only
__device__ inline uint64_t f64_round_bits(uint64_t a2, uint64_t a1, uint64_t a0, int e) {
  if (e > 1023) return kF64Inf;
  int shift = 11;                       // 64 - 53 kept bits
  if (e < -1022) {                      // subnormal: fewer kept bits
    shift += -1022 - e;
    if (shift > 64) return 0;           // below half the smallest subnormal
  }
  uint64_t m, rb, st;
  if (shift == 64) {
    m = 0;
    rb = a2 >> 63;
    st = a2 << 1;
  } else {
    m = a2 >> shift;
    rb = (a2 >> (shift - 1)) & 1;
    st = a2 << (65 - shift);
  }
  st |= a1 | a0;
  m += rb & (uint64_t)((st != 0) | (m & 1));
  if (e < -1022) return m;              // m == 2^52 is the smallest normal: the same bits
  uint64_t be = (uint64_t)(e + 1023);
  if (m >> 53) {
    m >>= 1;
    ++be;
  }
  if (be >= 2047) return kF64Inf;
  return (be << 52) | (m & 0xFFFFFFFFFFFFFULL);
}

// the double nearest the lower (upper == false) or upper end of the bracket of
// w * 10^q; w != 0, kPow5MinQ <= q <= kPow5MaxQ
__device__ inline uint64_t f64_scale_bits(uint64_t w, int q, bool upper) {
  const int lz = __builtin_clzll(w);
  w <<= lz;
  const uint64_t th = kPow5[q - kPow5MinQ][0], tl = kPow5[q - kPow5MinQ][1];
  const unsigned __int128 ph = (unsigned __int128)w * th, pl = (unsigned __int128)w * tl;
  uint64_t a0 = (uint64_t)pl;
  uint64_t a1 = (uint64_t)ph + (uint64_t)(pl >> 64);
  uint64_t a2 = (uint64_t)(ph >> 64) + (a1 < (uint64_t)ph);
  // 5^q = (T + d) * 2^(b - 127), b = floor(log2 5^q) (scripts/gen_pow5_table.py checks the formula)
  int e = 64 + ((152170 * q) >> 16) + q - lz;
  if (upper && !(q >= 0 && q <= kPow5ExactMaxQ)) {
    if (++a1 == 0 && ++a2 == 0) {       // the bound reached 2^192
      a2 = 1ULL << 63;
      ++e;
    }
  }
  if (!(a2 >> 63)) {
    a2 = (a2 << 1) | (a1 >> 63);
    a1 = (a1 << 1) | (a0 >> 63);
    a0 <<= 1;
    --e;
  }
  return f64_round_bits(a2, a1, a0, e);
}

// little-endian big integer of fixed capacity; every operation is bounded by it
constexpr int kBigWords = 90;           // 2880 bits; the comparison needs < 2^2640
constexpr int kBigDigits = 774;         // > 768 + 1, a multiple of 9
struct BigU {
  uint32_t w[kBigWords];
  int n;
};

__device__ inline void big_muladd(BigU& b, uint32_t m, uint32_t a) {
  uint64_t c = a;
  for (int i = 0; i < b.n; ++i) {
    c += (uint64_t)b.w[i] * m;
    b.w[i] = (uint32_t)c;
    c >>= 32;
  }
  if (c && b.n < kBigWords) b.w[b.n++] = (uint32_t)c;
}

__device__ inline void big_mul_pow5(BigU& b, int64_t k) {
  for (; k >= 13; k -= 13) big_muladd(b, 1220703125u, 0);   // 5^13
  uint32_t m = 1;
  for (; k > 0; --k) m *= 5;
  if (m > 1) big_muladd(b, m, 0);
}

__device__ inline void big_shl(BigU& b, int64_t s) {
  const int ws = (int)(s >> 5), bs = (int)(s & 31);
  if (b.n == 0 || b.n + ws + 1 > kBigWords) return;
  b.w[b.n] = 0;
  for (int i = b.n; i >= 0; --i) {
    const uint64_t v = ((uint64_t)b.w[i] << bs) | (bs && i ? b.w[i - 1] >> (32 - bs) : 0);
    b.w[i + ws] = (uint32_t)v;
  }
  for (int i = 0; i < ws; ++i) b.w[i] = 0;
  b.n += ws + 1;
  while (b.n && !b.w[b.n - 1]) --b.n;
}

__device__ inline int big_cmp(const BigU& a, const BigU& b) {
  if (a.n != b.n) return a.n < b.n ? -1 : 1;
  for (int i = a.n - 1; i >= 0; --i)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
  return 0;
}

// Sign of (digits [p, pe) * 10^x) - (midpoint between the doubles of bits `lo` and lo + 1)
__device__ inline int f64_cmp_midpoint(uint64_t lo, const uint8_t* p, const uint8_t* pe, int64_t x) {
  BigU D, R;
  D.n = 0;
  int nd = 0;
  bool dot = false, sticky = false;
  uint32_t chunk = 0, cm = 1;
  for (; p < pe; ++p) {
    const uint8_t c = *p;
    if (c == '.') {
      dot = true;
      continue;
    }
    const unsigned d = (unsigned)c - '0';
    if (nd == 0 && d == 0) {
      if (dot) --x;
      continue;
    }
    if (nd < kBigDigits) {
      chunk = chunk * 10 + d;
      cm *= 10;
      ++nd;
      if (dot) --x;
      if (cm == 1000000000u) {
        big_muladd(D, cm, chunk);
        chunk = 0;
        cm = 1;
      }
    } else {
      sticky |= d != 0;
      if (!dot) ++x;
    }
  }
  if (cm > 1) big_muladd(D, cm, chunk);
  // the caller's bracket puts the value next to this midpoint, so -1110 < x < 310
  if (x > 400) return 1;
  if (x < -1200) return -1;
  const uint64_t be = lo >> 52, frac = lo & 0xFFFFFFFFFFFFFULL;
  const uint64_t m2 = 2 * (be ? frac | (1ULL << 52) : frac) + 1;   // midpoint = m2 * 2^k
  const int64_t k = (be ? (int64_t)be - 1075 : -1074) - 1;
  R.w[0] = (uint32_t)m2;
  R.w[1] = (uint32_t)(m2 >> 32);
  R.n = R.w[1] ? 2 : 1;
  // D * 5^x * 2^x  <>  R * 2^k
  if (x >= 0) big_mul_pow5(D, x);
  else big_mul_pow5(R, -x);
  if (x - k > 0) big_shl(D, x - k);
  else if (k - x > 0) big_shl(R, k - x);
  const int c = big_cmp(D, R);
  return c == 0 && sticky ? 1 : c;
}

__device__ __noinline__ static uint64_t f64_exact_bits(uint64_t lo, uint64_t hi, const uint8_t* p, const uint8_t* pe,
                                                int64_t x) {
  // lo <= answer <= hi; hi == lo + 1 (the bracket is far narrower than one ulp)
  for (; lo < hi; ++lo) {
    const int c = f64_cmp_midpoint(lo, p, pe, x);
    if (c < 0) return lo;
    if (c == 0) return lo + (lo & 1);
  }
  return hi;
}

__device__ inline bool parse_f64(const uint8_t* p, const uint8_t* e, double* out) {
  bool neg = false;
  if (p < e && (*p == '-' || *p == '+')) neg = *p++ == '-';
  if (p >= e) return false;
  uint64_t bits;
  const uint8_t c0 = *p | 0x20;
  if (c0 == 'i' || c0 == 'n') {
    // the spellings Arrow and DataFusion read, any case
    if (ieq(p, e, "inf") || ieq(p, e, "infinity")) bits = kF64Inf;
    else if (ieq(p, e, "nan")) bits = kF64NaN;
    else return false;
  } else {
    const uint8_t* dstart = p;
    // integers, not flags, in the loop: lanes diverge here, and a flag carried
    // through divergent code costs a mask merge per iteration
    uint64_t w = 0;
    int sig = 0;            // significant digits in w
    int64_t nd = 0;         // digits seen
    int64_t nkept = 0;      // digits folded into w, leading zeros included
    int64_t nint = -1;      // digits before the point, -1: no point yet
    unsigned dropped = 0;   // OR of the digits that did not fit
    for (; p < e; ++p) {
      const uint8_t c = *p;
      const unsigned d = (unsigned)c - '0';
      if (d <= 9) {
        if (sig < 19) {
          w = w * 10 + d;
          sig += w != 0;
          ++nkept;
        } else {
          dropped |= d;
        }
        ++nd;
      } else if (c == '.' && nint < 0) {
        nint = nd;
      } else {
        break;              // a second point ends the digits and is no exponent mark: rejected below
      }
    }
    if (nd == 0) return false;
    const bool trunc = dropped != 0;
    if (nint < 0) nint = nd;
    // kept digits after the point scale down, dropped digits before it scale up
    int64_t e10 = nint - nkept;
    const uint8_t* dend = p;
    int64_t x = 0;
    if (p < e) {
      if ((*p | 0x20) != 'e') return false;
      ++p;
      bool xneg = false;
      if (p < e && (*p == '-' || *p == '+')) xneg = *p++ == '-';
      if (p >= e) return false;
      for (; p < e; ++p) {
        const unsigned d = (unsigned)*p - '0';
        if (d > 9) return false;
        if (x < ((int64_t)1 << 40)) x = x * 10 + d;   // clamped, never rejected
      }
      if (xneg) x = -x;
      e10 += x;
    }
    if (w == 0) {
      bits = 0;
    } else if (!trunc && w < (1ULL << 53) && e10 >= -22 && e10 <= 22) {
      // exact: both factors are representable, one rounding
      const double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                              1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
      double v = (double)w;
      if (e10 > 0) v *= p10[e10];
      else if (e10 < 0) v /= p10[-e10];
      *out = neg ? -v : v;
      return true;
    } else if (e10 > kPow5MaxQ) {
      bits = kF64Inf;                   // w >= 1
    } else if (e10 < kPow5MinQ) {
      bits = 0;                         // (w + 1) * 10^e10 <= 10^-325, below half the smallest subnormal
    } else {
      const uint64_t lo = f64_scale_bits(w, (int)e10, false);
      const uint64_t hi = f64_scale_bits(w + trunc, (int)e10, true);
      bits = lo == hi ? lo : f64_exact_bits(lo, hi, dstart, dend, x);
    }
  }
  if (neg) bits |= 1ULL << 63;
  double v;
  __builtin_memcpy(&v, &bits, sizeof v);
  *out = v;
  return true;
}

__device__ inline bool parse_date(const uint8_t* p, const uint8_t* e, int32_t* out) {
  if (e - p != 10 || p[4] != '-' || p[7] != '-') return false;
  int64_t y = 0, m = 0, d = 0;
  for (int k = 0; k < 4; ++k) {
    const unsigned c = (unsigned)p[k] - '0';
    if (c > 9) return false;
    y = y * 10 + c;
  }
  for (int k = 5; k < 7; ++k) {
    const unsigned c = (unsigned)p[k] - '0';
    if (c > 9) return false;
    m = m * 10 + c;
  }
  for (int k = 8; k < 10; ++k) {
    const unsigned c = (unsigned)p[k] - '0';
    if (c > 9) return false;
    d = d * 10 + c;
  }
  if (m < 1 || m > 12 || d < 1) return false;
  const bool leap = y % 4 == 0 && (y % 100 != 0 || y % 400 == 0);
  const int64_t dim = m == 2 ? (leap ? 29 : 28) : (m == 4 || m == 6 || m == 9 || m == 11) ? 30 : 31;
  if (d > dim) return false;
  *out = (int32_t)days_from_civil(y, m, d);
  return true;
}

// two ASCII digits at p -> 0..99, or -1
__device__ inline int parse_2digits(const uint8_t* p) {
  const unsigned a = (unsigned)p[0] - '0', b = (unsigned)p[1] - '0';
  return (a > 9 || b > 9) ? -1 : (int)(a * 10 + b);
}

// Naive timestamp text -> microseconds since 1970-01-01T00:00:00:
//   YYYY-MM-DD [ ('T' | 't' | ' ') HH:MM [ :SS [ .f{1,9} ] ] ] [ 'Z' | 'z' | +-HH | +-HH:MM | +-HHMM ]
// Years 0001-9999, a real calendar day, HH <= 23, MM and SS <= 59 (no leap second), offset
// hours <= 23 and minutes <= 59. Fraction digits past the sixth are dropped; an offset shifts
// the instant to UTC. Every field sits at a fixed position once the date is read; any other
// byte, before, between or after, rejects the text.
__device__ inline bool parse_timestamp(const uint8_t* p, const uint8_t* e, int64_t* out) {
  const int64_t n = e - p;
  int32_t days = 0;
  if (n < 10 || !parse_date(p, p + 10, &days)) return false;
  if (p[0] == '0' && p[1] == '0' && p[2] == '0' && p[3] == '0') return false;
  int64_t pos = 10, secs = 0, frac = 0;
  if (pos < n && (p[pos] == 'T' || p[pos] == 't' || p[pos] == ' ')) {
    if (n < pos + 6 || p[pos + 3] != ':') return false;
    const int hh = parse_2digits(p + pos + 1), mi = parse_2digits(p + pos + 4);
    if (hh < 0 || hh > 23 || mi < 0 || mi > 59) return false;
    secs = hh * 3600 + mi * 60;
    pos += 6;
    if (pos < n && p[pos] == ':') {
      if (n < pos + 3) return false;
      const int ss = parse_2digits(p + pos + 1);
      if (ss < 0 || ss > 59) return false;
      secs += ss;
      pos += 3;
      if (pos < n && p[pos] == '.') {
        ++pos;
        int nd = 0;
        int64_t unit = 100000;
        for (; pos < n && nd < 9; ++pos, ++nd) {
          const unsigned d = (unsigned)p[pos] - '0';
          if (d > 9) break;
          frac += d * unit;               // unit reaches 0 after six digits: the rest is dropped
          unit /= 10;
        }
        if (nd == 0) return false;
      }
    }
  }
  int64_t shift = 0;
  if (pos < n) {
    const uint8_t c = p[pos];
    const int64_t rest = n - pos - 1;
    if (c == 'Z' || c == 'z') {
      if (rest != 0) return false;
    } else if (c == '+' || c == '-') {
      if (rest != 2 && rest != 4 && rest != 5) return false;
      if (rest == 5 && p[pos + 3] != ':') return false;
      const int oh = parse_2digits(p + pos + 1);
      const int om = rest == 2 ? 0 : parse_2digits(p + pos + (rest == 5 ? 4 : 3));
      if (oh < 0 || oh > 23 || om < 0 || om > 59) return false;
      shift = oh * 3600 + om * 60;
      if (c == '-') shift = -shift;
    } else {
      return false;
    }
  }
  *out = ((int64_t)days * 86400 + secs - shift) * 1000000 + frac;
  return true;
}

// days since 1970-01-01 -> civil date (H. Hinnant's algorithm)
__device__ inline void civil_from_days(int64_t z, int64_t* y, int* m, int* d) {
  z += 719468;
  const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  const int64_t doe = z - era * 146097;
  const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  const int64_t mp = (5 * doy + 2) / 153;
  *d = (int)(doy - (153 * mp + 2) / 5 + 1);
  *m = (int)(mp < 10 ? mp + 3 : mp - 9);
  *y = yoe + era * 400 + (*m <= 2);
}

__device__ inline int u64_digits(uint64_t v) {
  int n = 1;
  while (v >= 10) {
    v /= 10;
    ++n;
  }
  return n;
}

// Text of a fixed-point value v * 10^-scale ("-12.05"; scale 0: an integer);
// returns the byte count, writes it when out != nullptr.
__device__ inline int format_fixed(int64_t v, int scale, uint8_t* out) {
  const bool neg = v < 0;
  const uint64_t u = neg ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
  int digits = u64_digits(u);
  if (digits <= scale) digits = scale + 1;          // leading "0."
  const int len = (int)neg + digits + (scale > 0 ? 1 : 0);
  if (out) {
    uint64_t x = u;
    int pos = len - 1;
    for (int k = 0; k < scale; ++k) {
      out[pos--] = (uint8_t)('0' + x % 10);
      x /= 10;
    }
    if (scale > 0) out[pos--] = '.';
    do {
      out[pos--] = (uint8_t)('0' + x % 10);
      x /= 10;
    } while (x && pos >= (int)neg);
    while (pos >= (int)neg) out[pos--] = '0';
    if (neg) out[0] = '-';
  }
  return len;
}

// YYYY-MM-DD of a date32 (years 0000-9999; others as their decimal year)
__device__ inline int format_date(int32_t days, uint8_t* out) {
  int64_t y;
  int m, d;
  civil_from_days(days, &y, &m, &d);
  if (y < 0 || y > 9999) {
    const int n = format_fixed(y, 0, out);
    if (out) {
      out[n] = '-';
      out[n + 1] = (uint8_t)('0' + m / 10);
      out[n + 2] = (uint8_t)('0' + m % 10);
      out[n + 3] = '-';
      out[n + 4] = (uint8_t)('0' + d / 10);
      out[n + 5] = (uint8_t)('0' + d % 10);
    }
    return n + 6;
  }
  if (out) {
    out[0] = (uint8_t)('0' + y / 1000);
    out[1] = (uint8_t)('0' + y / 100 % 10);
    out[2] = (uint8_t)('0' + y / 10 % 10);
    out[3] = (uint8_t)('0' + y % 10);
    out[4] = '-';
    out[5] = (uint8_t)('0' + m / 10);
    out[6] = (uint8_t)('0' + m % 10);
    out[7] = '-';
    out[8] = (uint8_t)('0' + d / 10);
    out[9] = (uint8_t)('0' + d % 10);
  }
  return 10;
}

}  // namespace kern
}  // namespace igloo
