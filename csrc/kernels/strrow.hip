// Byte-wise three-way compare of two string operands per row over plain
// (offsets + bytes) UTF-8 columns: the order behind greatest / least over
// strings (ops/strrow.py compare_rows).
//
// Operands follow strpair.hip: each side is (offsets, bytes, broadcast); a
// one-row column with broadcast = true serves a constant. One lane per row,
// grid-stride; a lane never indexes outside its rows' [off[i], off[i+1]).
// Bytes compare unsigned, which for UTF-8 is code point order; a string that
// is a prefix of the other sorts first.
// Parity: DataFusion's greatest / least (datafusion-functions 48, reference
// Cargo.lock:1062), reached through SessionContext::sql (reference
// crates/engine/src/lib.rs:54-57).
#include "common.h"
#include "kernels.h"

namespace igloo {
namespace kern {

namespace {

struct StrOp {
  const int64_t* off;
  const uint8_t* chars;
  bool bc;
};

struct Str {
  const uint8_t* p;
  int64_t n;
};

__device__ __forceinline__ Str row_str(const StrOp& o, int64_t i) {
  const int64_t r = o.bc ? 0 : i;
  const int64_t b = o.off[r];
  return Str{o.chars + b, o.off[r + 1] - b};
}

__global__ __launch_bounds__(kBlock) void str_row_cmp_kernel(StrOp a, StrOp b, int64_t n, int32_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const Str x = row_str(a, i), y = row_str(b, i);
    const int64_t m = x.n < y.n ? x.n : y.n;
    int32_t v = x.n < y.n ? -1 : x.n > y.n ? 1 : 0;      // a shorter prefix sorts first
    for (int64_t q = 0; q < m; ++q) {
      if (x.p[q] != y.p[q]) {
        v = x.p[q] < y.p[q] ? -1 : 1;
        break;
      }
    }
    out[i] = v;
  }
}

}  // namespace

void str_row_cmp(const int64_t* oa, const uint8_t* ca, bool ba, const int64_t* ob, const uint8_t* cb, bool bb, int64_t n,
                 int32_t* out, hipStream_t s) {
  if (n == 0) return;
  if (!oa || !ob) throw std::runtime_error("str_row_cmp: missing operand");
  hipLaunchKernelGGL(str_row_cmp_kernel, dim3(grid_for(n, kBlock, 1 << 16)), dim3(kBlock), 0, s, StrOp{oa, ca, ba},
                     StrOp{ob, cb, bb}, n, out);
  check_launch("strrow.cmp", s);
}

}  // namespace kern
}  // namespace igloo
