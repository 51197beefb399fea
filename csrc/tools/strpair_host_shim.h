// Host stand-in for common.h: lets csrc/tools/strpair_host.cpp compile the device routines of
// strpair.hip / strfunc.hip as plain C++ (one "thread" after another) under ASan / UBSan.
// tests/test_strpair_host.py copies it next to copies of the two kernel files as common.h;
// csrc/tools/textparse_host.cpp (tests/test_textparse_host.py) uses it the same way for textparse.h,
// csrc/tools/binary_host.cpp (tests/test_binary_host.py) for binary.hip and digest.hip,
// csrc/tools/winselect_host.cpp (tests/test_winselect_host.py) for window_select.h.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __constant__
#define __noinline__ __attribute__((noinline))
#define __shared__ static
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1) : x(a), y(1), z(1) {} };
static dim3 blockIdx, threadIdx, blockDim, gridDim;
typedef void* hipStream_t;
#define hipLaunchKernelGGL(...) ((void)0)
inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { auto o = *p; *p += v; return o; }
inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { auto o = *p; if (v > o) *p = v; return o; }
inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) { auto o = *p; if (v < o) *p = v; return o; }
// one "thread" after another: a barrier is a no-op, so kernels that share LDS run with blockDim.x == 1
// (csrc/tools/binary_host.cpp) and a block-wide vote is this thread's own
inline void __syncthreads() {}
inline int __syncthreads_or(int p) { return p; }
namespace igloo { namespace kern {
constexpr int kWave = 64; constexpr int kBlock = 256;
inline unsigned grid_for(int64_t n, int per, int64_t mx = 1 << 20) { return 1; }
inline void check_launch(const char*, hipStream_t) {}
}}
