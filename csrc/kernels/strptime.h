// to_timestamp(s, fmt...) / to_date(s, fmt...): one text parsed by a compiled list of
// chrono-style formats (the inverse of strfmt.hip). The host compiler
// (igloo_amd/ops/strptime.py compile_formats) turns the formats into one flat op
// program; parse_by_program interprets it over one row's bytes. The grammar is the
// table in the README ("Parsing dates and timestamps by format"); the Python twin
// py_strptime implements the same table on its own.
//
// Program: the formats one after another, each a run of ops closed by kOpEnd.
//   kOpLit n b0..b(n-1)   the n bytes themselves
//   every other op        one byte
// The formats are tried in order; the first that consumes the whole text and passes
// the range checks gives the value. Field state is a handful of scalars (no local
// arrays), so the kernel that includes this needs no scratch. Compiles as host C++
// through csrc/tools/strpair_host_shim.h (csrc/tools/strptime_host.cpp).
#pragma once
#include "textparse.h"

namespace igloo {
namespace kern {

enum StrptimeOp : uint8_t {
  kOpEnd = 0, kOpLit, kOpYear, kOpCent, kOpYy, kOpMon, kOpDay, kOpDaySp, kOpHour, kOpHourSp, kOpH12, kOpH12Sp,
  kOpMin, kOpSec, kOpDoy, kOpMonName, kOpWday, kOpAmPm, kOpNanos, kOpFracOpt, kOpFrac3, kOpFrac6, kOpFrac9,
  kOpOffset, kOpOffsetZ, kOpEpoch, kOpCount
};
// what the parsed instant is floored to: microseconds, milliseconds, seconds (all as int64
// microseconds) or the day number (to_date)
enum StrptimeUnit : int { kUnitMicros = 0, kUnitMillis = 1, kUnitSeconds = 2, kUnitDay = 3 };

constexpr int kMaxProgram = 256;
// 0001-01-01T00:00:00 .. 9999-12-31T23:59:59 in epoch seconds (the bound of %s)
constexpr int64_t kMinEpochS = -62135596800LL, kMaxEpochS = 253402300799LL;

// lowercase names in 9-byte slots, padded with spaces
static __constant__ const char kSpMonths[] =
    "january  february march    april    may      june     july     august   septemberoctober  november december ";
static __constant__ const char kSpDays[] = "sunday   monday   tuesday  wednesdaythursday friday   saturday ";
static_assert(sizeof(kSpMonths) == 12 * 9 + 1 && sizeof(kSpDays) == 7 * 9 + 1, "9-byte name slots");

// up to maxd digits, greedy: the count read (0: none)
__device__ inline int sp_digits(const uint8_t* p, const uint8_t* e, int maxd, int64_t* v) {
  int k = 0;
  int64_t x = 0;
  while (k < maxd && p + k < e && (unsigned)(p[k] - '0') <= 9u) {
    x = x * 10 + (p[k] - '0');
    ++k;
  }
  *v = x;
  return k;
}

// a name of the 9-byte-slot table at p, ASCII case-insensitive: full names first, then the
// three-letter forms. Returns the bytes consumed (0: none) and the entry in *which.
__device__ inline int sp_name(const uint8_t* p, const uint8_t* e, const char* table, int count, int* which) {
  for (int pass = 0; pass < 2; ++pass) {
    for (int k = 0; k < count; ++k) {
      const char* nm = table + 9 * k;
      int len = 3;
      if (pass == 0) {
        len = 9;
        while (nm[len - 1] == ' ') --len;
      }
      if (e - p < len) continue;
      int j = 0;
      while (j < len && (uint8_t)(p[j] | 0x20) == (uint8_t)nm[j]) ++j;
      if (j == len) {
        *which = k;
        return len;
      }
    }
  }
  return 0;
}

__device__ inline int64_t sp_floor_div(int64_t a, int64_t b) {
  int64_t q = a / b;
  return (a % b != 0 && (a < 0)) ? q - 1 : q;
}

// One format of the program starting at prog[pc] (ends at its kOpEnd) over [p, e).
// Returns 1 on a match (value in *out), 0 on a non-match, -1 on a malformed program.
__device__ inline int sp_try_format(const uint8_t* p, const uint8_t* e, const uint8_t* prog, int plen, int pc,
                                    int unit, int64_t* out) {
  int year = -1, cent = -1, yy = -1, mon = -1, day = -1, doy = -1, hour = 0, h12 = -1, pm = -1, mi = 0, sec = 0;
  int wday = -1, off = 0;
  bool has_epoch = false;
  int64_t epoch = 0, ns = 0, v = 0;
  for (;;) {
    if (pc >= plen) return -1;
    const uint8_t op = prog[pc++];
    if (op == kOpEnd) break;
    int k;
    switch (op) {
      case kOpLit: {
        if (pc >= plen) return -1;
        const int n = prog[pc++];
        if (pc + n > plen) return -1;
        if (e - p < n) return 0;
        for (int j = 0; j < n; ++j)
          if (p[j] != prog[pc + j]) return 0;
        p += n;
        pc += n;
        break;
      }
      case kOpYear:
        k = sp_digits(p, e, 4, &v);
        if (!k || v < 1) return 0;
        year = (int)v;
        p += k;
        break;
      case kOpCent:
      case kOpYy:
      case kOpMon:
      case kOpDay:
      case kOpHour:
      case kOpH12:
      case kOpMin:
      case kOpSec:
      case kOpDaySp:
      case kOpHourSp:
      case kOpH12Sp: {
        if ((op == kOpDaySp || op == kOpHourSp || op == kOpH12Sp) && p < e && *p == ' ') ++p;
        k = sp_digits(p, e, 2, &v);
        if (!k) return 0;
        p += k;
        const int x = (int)v;
        if (op == kOpCent) cent = x;
        else if (op == kOpYy) yy = x;
        else if (op == kOpMon) { if (x < 1 || x > 12) return 0; mon = x; }
        else if (op == kOpDay || op == kOpDaySp) { if (x < 1 || x > 31) return 0; day = x; }
        else if (op == kOpHour || op == kOpHourSp) { if (x > 23) return 0; hour = x; }
        else if (op == kOpH12 || op == kOpH12Sp) { if (x < 1 || x > 12) return 0; h12 = x; }
        else if (op == kOpMin) { if (x > 59) return 0; mi = x; }
        else { if (x > 59) return 0; sec = x; }
        break;
      }
      case kOpDoy:
        k = sp_digits(p, e, 3, &v);
        if (!k || v < 1 || v > 366) return 0;
        doy = (int)v;
        p += k;
        break;
      case kOpMonName:
        k = sp_name(p, e, kSpMonths, 12, &mon);
        if (!k) return 0;
        mon += 1;
        p += k;
        break;
      case kOpWday:
        k = sp_name(p, e, kSpDays, 7, &wday);
        if (!k) return 0;
        p += k;
        break;
      case kOpAmPm:
        if (e - p < 2 || (p[1] | 0x20) != 'm') return 0;
        if ((p[0] | 0x20) == 'a') pm = 0;
        else if ((p[0] | 0x20) == 'p') pm = 1;
        else return 0;
        p += 2;
        break;
      case kOpNanos:
        k = sp_digits(p, e, 9, &ns);
        if (!k) return 0;
        p += k;
        break;
      case kOpFracOpt:
      case kOpFrac3:
      case kOpFrac6:
      case kOpFrac9: {
        const int want = op == kOpFrac3 ? 3 : op == kOpFrac6 ? 6 : 9;
        if (op == kOpFracOpt && !(e - p >= 2 && p[0] == '.' && (unsigned)(p[1] - '0') <= 9u)) break;   // absent: 0
        if (p >= e || *p != '.') return 0;
        ++p;
        k = sp_digits(p, e, want, &ns);
        if (!k || (op != kOpFracOpt && k != want)) return 0;
        p += k;
        for (int j = k; j < 9; ++j) ns *= 10;      // left-aligned
        break;
      }
      case kOpOffset:
      case kOpOffsetZ: {
        if (op == kOpOffsetZ && p < e && (*p | 0x20) == 'z') {
          off = 0;
          ++p;
          break;
        }
        if (p >= e || (*p != '+' && *p != '-')) return 0;
        const bool neg = *p == '-';
        ++p;
        if (e - p < 2 || (unsigned)(p[0] - '0') > 9u || (unsigned)(p[1] - '0') > 9u) return 0;
        const int oh = (p[0] - '0') * 10 + (p[1] - '0');
        p += 2;
        int om = -1;
        const uint8_t* q = (p < e && *p == ':') ? p + 1 : p;
        if (e - q >= 2 && (unsigned)(q[0] - '0') <= 9u && (unsigned)(q[1] - '0') <= 9u) {
          om = (q[0] - '0') * 10 + (q[1] - '0');
          p = q + 2;
        }
        if (om < 0) {
          if (op != kOpOffsetZ) return 0;        // +HH alone is %#z only
          om = 0;
        }
        if (oh > 23 || om > 59) return 0;
        off = (oh * 3600 + om * 60) * (neg ? -1 : 1);
        break;
      }
      case kOpEpoch: {
        const bool neg = p < e && *p == '-';
        if (neg) ++p;
        k = sp_digits(p, e, 18, &epoch);
        if (!k) return 0;
        p += k;
        if (neg) epoch = -epoch;
        if (epoch < kMinEpochS || epoch > kMaxEpochS) return 0;
        has_epoch = true;
        break;
      }
      default: return -1;
    }
  }
  if (p != e) return 0;
  int64_t secs;
  if (has_epoch) {
    secs = epoch;
  } else {
    if (year < 0) {
      if (yy < 0) return -1;
      year = cent >= 0 ? cent * 100 + yy : (yy <= 68 ? 2000 + yy : 1900 + yy);
      if (yy > 99 || year < 1 || year > 9999) return 0;
    }
    const bool leap = (year % 4 == 0 && year % 100 != 0) || year % 400 == 0;
    int64_t days;
    if (doy >= 0) {
      if (doy > (leap ? 366 : 365)) return 0;
      days = days_from_civil(year, 1, 1) + doy - 1;
    } else {
      if (mon < 0 || day < 0) return -1;
      const int mdays = mon == 2 ? (leap ? 29 : 28) : (mon == 4 || mon == 6 || mon == 9 || mon == 11) ? 30 : 31;
      if (day > mdays) return 0;
      days = days_from_civil(year, mon, day);
    }
    if (wday >= 0 && (int)(((days % 7) + 11) % 7) != wday) return 0;     // 1970-01-01 was a Thursday
    if (h12 >= 0) {
      if (pm < 0) return -1;
      hour = h12 % 12 + (pm ? 12 : 0);
    }
    secs = days * 86400 + hour * 3600 + mi * 60 + sec - off;
  }
  const int64_t us = ns / 1000;           // digits past the sixth are dropped
  if (unit == kUnitDay) *out = sp_floor_div(secs, 86400);
  else if (unit == kUnitSeconds) *out = secs * 1000000;
  else if (unit == kUnitMillis) *out = secs * 1000000 + us / 1000 * 1000;
  else *out = secs * 1000000 + us;
  return 1;
}

// The text [p, e) by the program: true and the value in *out for the first format that
// matches, false (out untouched) when none does or the program is malformed.
__device__ inline bool parse_by_program(const uint8_t* p, const uint8_t* e, const uint8_t* prog, int plen, int unit,
                                        int64_t* out) {
  if (plen > kMaxProgram) return false;
  int pc = 0;
  while (pc < plen) {
    const int r = sp_try_format(p, e, prog, plen, pc, unit, out);
    if (r != 0) return r > 0;
    // skip to the next format
    for (;;) {
      if (pc >= plen) return false;
      const uint8_t op = prog[pc++];
      if (op == kOpEnd) break;
      if (op == kOpLit) {
        if (pc >= plen) return false;
        pc += 1 + prog[pc];
      }
    }
  }
  return false;
}

}  // namespace kern
}  // namespace igloo
