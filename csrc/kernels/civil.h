// Proleptic-Gregorian calendar helpers shared by the date / time-zone kernels
// (days are counted from 1970-01-01).
#pragma once

#include "common.h"

namespace igloo {
namespace kern {

__device__ inline void civil(int64_t z0, int* y, int* m, int* d) {
  int64_t z = z0 + 719468;
  int64_t era = (z >= 0 ? z : z - 146096) / 146097;
  int64_t doe = z - era * 146097;
  int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
  int64_t yy = yoe + era * 400;
  int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
  int64_t mp = (5 * doy + 2) / 153;
  int64_t dd = doy - (153 * mp + 2) / 5 + 1;
  int64_t mm = mp < 10 ? mp + 3 : mp - 9;
  *y = (int)(yy + (mm <= 2));
  *m = (int)mm;
  *d = (int)dd;
}

__device__ inline int64_t days_from_civil(int64_t y, int m, int d) {
  y -= m <= 2;
  int64_t era = (y >= 0 ? y : y - 399) / 400;
  int64_t yoe = y - era * 400;
  int64_t doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
  int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}

}  // namespace kern
}  // namespace igloo
