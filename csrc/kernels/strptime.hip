// to_timestamp(s, fmt...) / to_date(s, fmt...) on the device: one lane per row runs the
// compiled format program of strptime.h over the row's bytes (grid-stride, like strfmt).
// The program travels by value in the kernel arguments: every lane reads it from the
// kernel-argument segment, so there is no LDS and no global table. A row whose byte range
// is negative, reversed or reaches past nbytes is a failed row and its bytes are not read.
// A failed non-NULL row writes 0 and leaves its index in err[0] by atomicMin (the cell
// starts at n); the host reads it back once and names the row.
#include "common.h"
#include "kernels.h"
#include "strptime.h"

namespace igloo {
namespace kern {

namespace {

struct StrptimeArgs {
  uint8_t prog[kMaxProgram];
  int plen;
  int unit;
};

__global__ __launch_bounds__(kBlock) void strptime_kernel(StrptimeArgs a, const int64_t* __restrict__ off,
                                                        const uint8_t* __restrict__ chars, int64_t nbytes,
                                                        const uint8_t* __restrict__ valid, int64_t n,
                                                        void* __restrict__ out, unsigned long long* __restrict__ err) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t v = 0;
    if (valid == nullptr || valid[r]) {
      const int64_t b = off[r], e = off[r + 1];
      const bool ok = b >= 0 && e >= b && e <= nbytes && parse_by_program(chars + b, chars + e, a.prog, a.plen, a.unit, &v);
      if (!ok) {
        v = 0;
        atomicMin(err, (unsigned long long)r);
      }
    }
    if (a.unit == kUnitDay) ((int32_t*)out)[r] = (int32_t)v;
    else ((int64_t*)out)[r] = v;
  }
}

}  // namespace

void strptime(const uint8_t* prog, int plen, int unit, const int64_t* off, const uint8_t* chars, int64_t nbytes,
              const uint8_t* valid, int64_t n, void* out, int64_t* err, hipStream_t s) {
  if (plen < 0 || plen > kMaxProgram) throw std::runtime_error("strptime: program longer than 256 bytes");
  if (unit < kUnitMicros || unit > kUnitDay) throw std::runtime_error("strptime: unknown unit");
  if (n == 0) return;
  StrptimeArgs a;
  for (int i = 0; i < kMaxProgram; ++i) a.prog[i] = i < plen ? prog[i] : (uint8_t)kOpEnd;
  a.plen = plen;
  a.unit = unit;
  hipLaunchKernelGGL(strptime_kernel, dim3(grid_for(n, kBlock, 1 << 14)), dim3(kBlock), 0, s, a, off, chars, nbytes,
                     valid, n, out, reinterpret_cast<unsigned long long*>(err));
  check_launch("strptime", s);
}

}  // namespace kern
}  // namespace igloo
