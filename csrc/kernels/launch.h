// Host-side launch helpers: turn runtime width / mode flags into template
// arguments once, and derive every pointer cast from the same tag.
//
//   dispatch(wide{key64}, direct, wide{rid64}, [&](auto k, auto d, auto r) {
//     using K = type_of<decltype(k)>;
//     using R = type_of<decltype(r)>;
//     launch("join_build", join_build_kernel<K, d.value, R>, g, b, 0, stream, as<K>(keys), ..., as<R>(thead), ...);
//   });
#pragma once

#include <type_traits>

#include "common.h"

namespace igloo {
namespace kern {

template <typename T> struct tag { using type = T; };
template <typename Tag> using type_of = typename Tag::type;

struct wide { bool is64; };   // -> tag<int32_t> / tag<int64_t>
struct uwide { bool is64; };  // -> tag<uint32_t> / tag<uint64_t>
                              // a plain bool -> std::false_type / std::true_type
struct value_bytes { int n; };  // 0 (no values), 1, 2 or 4 -> std::integral_constant<int, n>

template <typename F> void pick(wide w, F&& f) { w.is64 ? f(tag<int64_t>{}) : f(tag<int32_t>{}); }
template <typename F> void pick(uwide w, F&& f) { w.is64 ? f(tag<uint64_t>{}) : f(tag<uint32_t>{}); }
template <typename F> void pick(bool b, F&& f) { b ? f(std::true_type{}) : f(std::false_type{}); }
template <typename F> void pick(value_bytes b, F&& f) {
  using std::integral_constant;
  b.n == 0 ? f(integral_constant<int, 0>{}) : b.n == 1 ? f(integral_constant<int, 1>{})
  : b.n == 2 ? f(integral_constant<int, 2>{}) : f(integral_constant<int, 4>{});
}

// dispatch(flags..., f): call f with one tag per flag
template <typename A, typename F> void dispatch(A a, F&& f) { pick(a, f); }
template <typename A, typename B, typename F> void dispatch(A a, B b, F&& f) {
  pick(a, [&](auto x) { pick(b, [&](auto y) { f(x, y); }); });
}
template <typename A, typename B, typename C, typename F> void dispatch(A a, B b, C c, F&& f) {
  pick(a, [&](auto x) { dispatch(b, c, [&](auto y, auto z) { f(x, y, z); }); });
}
template <typename A, typename B, typename C, typename D, typename F> void dispatch(A a, B b, C c, D d, F&& f) {
  pick(a, [&](auto x) { dispatch(b, c, d, [&](auto y, auto z, auto w) { f(x, y, z, w); }); });
}

template <typename T> T* as(void* p) { return static_cast<T*>(p); }
template <typename T> const T* as(const void* p) { return static_cast<const T*>(p); }

// launch + launch-error check under one name
template <typename... P, typename... Args>
void launch(const char* what, void (*kernel)(P...), dim3 grid, dim3 block, size_t shmem, hipStream_t stream,
            Args&&... args) {
  hipLaunchKernelGGL(kernel, grid, block, shmem, stream, args...);
  check_launch(what, stream);
}

}  // namespace kern
}  // namespace igloo
