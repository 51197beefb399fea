// LIST / STRUCT / MAP column helpers (DataFusion's datafusion-functions-nested,
// reference Cargo.lock:1125, reached through SessionContext::sql at
// crates/engine/src/lib.rs:54-57).
//
// A LIST row is an (start, length) pair into a child column, so most list
// work is index arithmetic followed by one gather of the child (gather.hip):
//   list_element_idx  child row of element i (1-based; negative counts from
//                     the end) per row, -1 = NULL (out of range / NULL row)
//   interleave_idx    make_array(c0..ck-1): child row r*k+j is c_j[r], read
//                     from the columns concatenated end to end (j*n + r)
//   list_slots        per-row (start, length) of a fixed-arity list
// Unnest uses expand_ranges (ranges.hip) over (start, length).
//
// The array_* function family (ops/nested.py has one function per SQL name):
//   list_slice_se     slot arithmetic: new (start, length) pairs over the SAME child
//                     (array_slice, l[a:b], array_pop_front / _back)
//   list_parts_*      k-way per-row concatenation of (start, length, stride) parts of one
//                     source column: append, prepend, concat, ||, resize with fill
//                     (stride 0 = a repeated row), repeat, reverse (stride -1)
//   list_flatten_*    one level of LIST<LIST<T>> through two levels of (start, length)
//   list_match_*      linear search over an int64 equality key per child element:
//                     position(s), has / = ANY with a per-row needle, remove / replace
//                     with a per-row limit;  list_minmax_idx: child row of the extreme
//   list_set_*        distinct, union, intersect, except, has_all, has_any: all-pairs
//                     compares of keys a wave staged in LDS
//   list_sort_idx     array_sort: bitonic sort of (null class, order key, position) in LDS
// Rebuild kernels run count -> exclusive scan (scan.hip) -> write and emit an int64 map
// of source rows (-1 = NULL) that one gather (gather.hip) turns into the new child; no
// element data moves before that gather. Rows may alias, overlap, start anywhere and
// leave child rows unreferenced: nothing here assumes lists tile the child, and every
// emitted row is checked against the child's length, every write against its buffer.
// MAP rows are the same (start, length) pairs over two equally long children (key, value), so
// map_keys / map_values / map_entries / cardinality need no kernel;
//   map_lookup_idx    m[k] / element_at / map_extract: child row of the first entry whose key
//                     equals a constant or per-row needle, keys compared where they lie (fixed
//                     width at their own size, plain UTF-8 by length, then dwords and a byte tail)
// Not here: a slice stride, array_dims, string_to_array, unnest(struct), unnest(map), ordering
// or equality of nested elements and maps (the binder answers NotSupported).
#include "common.h"
#include "kernels.h"

namespace igloo {
namespace kern {

namespace {

__global__ __launch_bounds__(kBlock) void list_element_idx_kernel(const int64_t* __restrict__ se,
                                                                const uint8_t* __restrict__ valid,
                                                                const int64_t* __restrict__ pos,
                                                                const uint8_t* __restrict__ pos_valid,
                                                                int64_t pos_const, int64_t n, int64_t child_n,
                                                                int64_t* __restrict__ out) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t start = se[2 * r], len = se[2 * r + 1];
    const int64_t i = pos ? pos[r] : pos_const;
    int64_t k = i > 0 ? i - 1 : len + i;          // 1-based from the front, -1 = last
    const bool ok = (!valid || valid[r]) && (!pos_valid || pos_valid[r]) && i != 0 && k >= 0 && k < len &&
                    start >= 0 && start + k < child_n;
    out[r] = ok ? start + k : -1;
  }
}

__global__ __launch_bounds__(kBlock) void interleave_idx_kernel(int64_t n, int k, int64_t* __restrict__ out) {
  const int64_t total = n * k;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / k, j = t - r * k;
    out[t] = j * n + r;
  }
}

__global__ __launch_bounds__(kBlock) void list_slots_kernel(int64_t n, int64_t k, int64_t* __restrict__ se) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    se[2 * r] = r * k;
    se[2 * r + 1] = k;
  }
}

// ---------------------------------------------------------------- list function family
// Schedule shared by the per-row kernels: a wave owns 64 consecutive rows. Rows whose work is at most
// `Short` elements run one lane per row; every longer row of the tile is then walked by the whole wave,
// one row after another, lanes striding its elements (ballot + popcount keep compacted output in order).
template <class F>
__device__ inline void for_wave_tiles(int64_t n, int64_t short_max, F& f) {
  const int lane = lane_id();
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
  const int64_t nwaves = (int64_t)gridDim.x * blockDim.x / kWave;
  for (int64_t tile = wave0; tile * kWave < n; tile += nwaves) {
    const int64_t r = tile * kWave + lane;
    const int64_t work = r < n ? f.work(r) : 0;
    if (r < n && work <= short_max) f.short_row(r);
    uint64_t longs = __ballot(r < n && work > short_max);
    while (longs) {
      const int l = __ffsll((unsigned long long)longs) - 1;
      longs &= longs - 1;
      f.long_row(tile * kWave + l, lane);
    }
  }
}

// Output positions come from offsets computed on the device while the buffer may have been sized from a
// replayed readback: every write is bounded by the buffer the launcher passed.
__device__ inline void put(int64_t* out, int64_t cap, int64_t pos, int64_t v) {
  if (pos >= 0 && pos < cap) out[pos] = v;
}

__device__ inline bool row_ok(const uint8_t* valid, int64_t r) { return !valid || valid[r]; }

// (start, length) of a row as the kernels walk it: nothing for a NULL row or a malformed slot
__device__ inline void row_range(const int64_t* se, const uint8_t* valid, int64_t r, int64_t& st, int64_t& ln) {
  st = se[2 * r];
  ln = se[2 * r + 1];
  if (!row_ok(valid, r) || ln < 0 || st < 0) ln = 0;
}

__global__ __launch_bounds__(kBlock) void list_slice_se_kernel(
    const int64_t* __restrict__ se, const uint8_t* __restrict__ valid, const int64_t* __restrict__ from,
    const uint8_t* __restrict__ from_valid, const int64_t* __restrict__ to, const uint8_t* __restrict__ to_valid,
    int64_t from_const, int64_t to_const, int64_t n, int64_t* __restrict__ out_se, uint8_t* __restrict__ out_valid) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t st = se[2 * r], ln = se[2 * r + 1] < 0 ? 0 : se[2 * r + 1];
    const bool ok = row_ok(valid, r) && row_ok(from_valid, r) && row_ok(to_valid, r);
    int64_t a = from ? from[r] : from_const, b = to ? to[r] : to_const;
    // 1-based inclusive -> 0-based [a, b]; negative counts from the end; clamp to the list
    a = a > 0 ? a - 1 : (a == 0 ? 0 : ln + a);
    b = b > 0 ? b - 1 : (b == 0 ? -1 : ln + b);
    if (a < 0) a = 0;
    if (b > ln - 1) b = ln - 1;
    const int64_t m = (ok && b >= a) ? b - a + 1 : 0;
    out_se[2 * r] = m ? st + a : 0;
    out_se[2 * r + 1] = m;
    out_valid[r] = ok;
  }
}

// ---- parts: k-way per-row concatenation ------------------------------------------
__device__ inline void part_of(const int64_t* parts, int64_t n, int j, int64_t r, int64_t& st, int64_t& ln,
                               int64_t& stride) {
  const int64_t* p = parts + ((int64_t)j * n + r) * 3;
  st = p[0];
  ln = p[1] < 0 ? 0 : p[1];
  stride = p[2];
}

__global__ __launch_bounds__(kBlock) void list_parts_count_kernel(const int64_t* __restrict__ parts, int k, int64_t n,
                                                                  int64_t* __restrict__ out_len) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    int64_t total = 0, st, ln, stride;
    for (int j = 0; j < k; ++j) {
      part_of(parts, n, j, r, st, ln, stride);
      total += ln;
    }
    out_len[r] = total;
  }
}

struct PartsWrite {
  const int64_t* parts;
  int k;
  int64_t n;
  const int64_t* offs;
  int64_t src_n;
  int64_t cap;
  int64_t* idx;
  int64_t* out_se;
  __device__ int64_t work(int64_t r) const { return offs[r + 1] - offs[r]; }
  __device__ int64_t src(int64_t st, int64_t t, int64_t stride) const {
    const int64_t v = st + t * stride;
    return (st >= 0 && v >= 0 && v < src_n) ? v : -1;
  }
  __device__ void short_row(int64_t r) const {
    int64_t o = offs[r], st, ln, stride;
    out_se[2 * r] = o;
    out_se[2 * r + 1] = offs[r + 1] - o;
    for (int j = 0; j < k; ++j) {
      part_of(parts, n, j, r, st, ln, stride);
      for (int64_t t = 0; t < ln; ++t) put(idx, cap, o++, src(st, t, stride));
    }
  }
  __device__ void long_row(int64_t r, int lane) const {
    int64_t o = offs[r], st, ln, stride;
    if (lane == 0) {
      out_se[2 * r] = o;
      out_se[2 * r + 1] = offs[r + 1] - o;
    }
    for (int j = 0; j < k; ++j) {
      part_of(parts, n, j, r, st, ln, stride);
      for (int64_t t = lane; t < ln; t += kWave) put(idx, cap, o + t, src(st, t, stride));
      o += ln;
    }
  }
};

__global__ __launch_bounds__(kBlock) void list_parts_write_kernel(PartsWrite f) { for_wave_tiles(f.n, kWave, f); }

// ---- flatten ---------------------------------------------------------------------
struct Flatten {
  const int64_t* se;
  const uint8_t* valid;
  const int64_t* ise;
  const uint8_t* ivalid;
  int64_t n, inner_n;
  const int64_t* offs;   // null: the count pass
  int64_t child_n;
  int64_t cap;
  int64_t* out;          // count pass: lengths; write pass: child rows
  int64_t* out_se;
  __device__ void inner(int64_t j, int64_t& st, int64_t& ln) const {
    st = ln = 0;
    if (j >= 0 && j < inner_n) row_range(ise, ivalid, j, st, ln);
  }
  __device__ int64_t work(int64_t r) const {
    if (offs) return offs[r + 1] - offs[r];
    int64_t st, ln;
    row_range(se, valid, r, st, ln);
    return ln;
  }
  __device__ void short_row(int64_t r) const {
    int64_t st, ln, ist, iln, total = 0;
    row_range(se, valid, r, st, ln);
    int64_t o = offs ? offs[r] : 0;
    for (int64_t j = 0; j < ln; ++j) {
      inner(st + j, ist, iln);
      total += iln;
      if (offs)
        for (int64_t t = 0; t < iln; ++t) put(out, cap, o++, ist + t < child_n ? ist + t : -1);
    }
    if (!offs) {
      out[r] = total;
    } else {
      out_se[2 * r] = offs[r];
      out_se[2 * r + 1] = total;
    }
  }
  __device__ void long_row(int64_t r, int lane) const {
    int64_t st, ln, ist, iln;
    row_range(se, valid, r, st, ln);
    if (!offs) {
      int64_t total = 0;
      for (int64_t j = lane; j < ln; j += kWave) {
        inner(st + j, ist, iln);
        total += iln;
      }
      total = wave_reduce_sum(total);
      if (lane == 0) out[r] = total;
      return;
    }
    int64_t o = offs[r];
    if (lane == 0) {
      out_se[2 * r] = o;
      out_se[2 * r + 1] = offs[r + 1] - o;
    }
    for (int64_t j = 0; j < ln; ++j) {
      inner(st + j, ist, iln);
      for (int64_t t = lane; t < iln; t += kWave) put(out, cap, o + t, ist + t < child_n ? ist + t : -1);
      o += iln;
    }
  }
};

__global__ __launch_bounds__(kBlock) void list_flatten_kernel(Flatten f) { for_wave_tiles(f.n, kWave, f); }

// ---- linear search over equality keys -----------------------------------------------
struct Match {
  const int64_t* se;
  const uint8_t* valid;
  const int64_t* keys;
  const uint8_t* kvalid;
  int64_t child_n;
  const int64_t* needle;
  const uint8_t* needle_valid;
  const int64_t* from;
  const int64_t* limit;
  int64_t limit_const;
  int mode;              // count: 0 position, 1 matches, 2 length after remove; write: 10 + (0 positions, 1 remove, 2 replace)
  int64_t n;
  const int64_t* offs;
  int64_t repl_base;
  int64_t cap;           // write modes: elements of out
  int64_t* out;
  __device__ int64_t work(int64_t r) const {
    int64_t st, ln;
    row_range(se, valid, r, st, ln);
    return ln;
  }
  // element t of a row is the child row st + t; out of range reads as NULL (as the gather does)
  __device__ bool hit(int64_t c, int64_t nk, bool nv) const {
    const bool ev = c < child_n && (!kvalid || kvalid[c]);
    return nv ? (ev && keys[c] == nk) : !ev;
  }
  __device__ int64_t lim(int64_t r) const {
    const int64_t l = limit ? limit[r] : limit_const;
    return l < 0 ? 0 : l;
  }
  __device__ int64_t row_of(int64_t c) const { return c < child_n ? c : -1; }
  __device__ void short_row(int64_t r) const {
    int64_t st, ln;
    row_range(se, valid, r, st, ln);
    const int64_t nk = needle[r];
    const bool nv = row_ok(needle_valid, r);
    if (mode == 0) {
      int64_t t0 = from ? from[r] - 1 : 0, pos = 0;
      if (t0 < 0) t0 = 0;
      for (int64_t t = t0; t < ln && !pos; ++t)
        if (hit(st + t, nk, nv)) pos = t + 1;
      out[r] = pos;
      return;
    }
    const int64_t L = lim(r);
    int64_t m = 0, o = offs ? offs[r] : 0;
    for (int64_t t = 0; t < ln; ++t) {
      const bool h = hit(st + t, nk, nv);
      if (mode == 10) {
        if (h) put(out, cap, o + m, t + 1);
      } else if (mode == 11) {
        if (!(h && m < L)) put(out, cap, o++, row_of(st + t));
      } else if (mode == 12) {
        put(out, cap, o + t, (h && m < L) ? repl_base + r : row_of(st + t));
      }
      m += h;
    }
    if (mode == 1) out[r] = m;
    if (mode == 2) out[r] = ln - (m < L ? m : L);
  }
  __device__ void long_row(int64_t r, int lane) const {
    int64_t st, ln;
    row_range(se, valid, r, st, ln);
    const int64_t nk = needle[r];
    const bool nv = row_ok(needle_valid, r);
    if (mode == 0) {
      int64_t t0 = from ? from[r] - 1 : 0, pos = 0;
      if (t0 < 0) t0 = 0;
      for (int64_t base = t0; base < ln && !pos; base += kWave) {
        const int64_t t = base + lane;
        const uint64_t hb = __ballot(t < ln && hit(st + t, nk, nv));
        if (hb) pos = base + __ffsll((unsigned long long)hb);
      }
      if (lane == 0) out[r] = pos;
      return;
    }
    const int64_t L = lim(r), o = offs ? offs[r] : 0;
    int64_t run_m = 0, run_o = 0;
    for (int64_t base = 0; base < ln; base += kWave) {
      const int64_t t = base + lane;
      const bool act = t < ln;
      const bool h = act && hit(st + t, nk, nv);
      const uint64_t hb = __ballot(h);
      const int64_t rank = run_m + lane_prefix(hb);
      if (mode == 10) {
        if (h) put(out, cap, o + rank, t + 1);
      } else if (mode == 11) {
        const bool keep = act && !(h && rank < L);
        const uint64_t kb = __ballot(keep);
        if (keep) put(out, cap, o + run_o + lane_prefix(kb), row_of(st + t));
        run_o += __popcll(kb);
      } else if (mode == 12) {
        if (act) put(out, cap, o + t, (h && rank < L) ? repl_base + r : row_of(st + t));
      }
      run_m += __popcll(hb);
    }
    if (lane == 0 && mode == 1) out[r] = run_m;
    if (lane == 0 && mode == 2) out[r] = ln - (run_m < L ? run_m : L);
  }
};

__global__ __launch_bounds__(kBlock) void list_match_kernel(Match f) { for_wave_tiles(f.n, kWave, f); }

struct MinMax {
  const int64_t* se;
  const uint8_t* valid;
  const int64_t* keys;
  const uint8_t* kvalid;
  int64_t child_n;
  bool is_max;
  int64_t n;
  int64_t* out;
  __device__ int64_t work(int64_t r) const {
    int64_t st, ln;
    row_range(se, valid, r, st, ln);
    return ln;
  }
  __device__ bool better(int64_t k, int64_t c, int64_t bk, int64_t bc) const {
    if (bc < 0) return true;
    if (k != bk) return is_max ? k > bk : k < bk;
    return c < bc;
  }
  __device__ void scan(int64_t st, int64_t ln, int64_t t0, int64_t step, int64_t& bk, int64_t& bc) const {
    for (int64_t t = t0; t < ln; t += step) {
      const int64_t c = st + t;
      if (c >= child_n || (kvalid && !kvalid[c])) continue;
      if (better(keys[c], c, bk, bc)) {
        bk = keys[c];
        bc = c;
      }
    }
  }
  __device__ void short_row(int64_t r) const {
    int64_t st, ln, bk = 0, bc = -1;
    row_range(se, valid, r, st, ln);
    scan(st, ln, 0, 1, bk, bc);
    out[r] = bc;
  }
  __device__ void long_row(int64_t r, int lane) const {
    int64_t st, ln, bk = 0, bc = -1;
    row_range(se, valid, r, st, ln);
    scan(st, ln, lane, kWave, bk, bc);
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const int64_t ok = __shfl_xor(bk, off, kWave), oc = __shfl_xor(bc, off, kWave);
      if (oc >= 0 && better(ok, oc, bk, bc)) {
        bk = ok;
        bc = oc;
      }
    }
    if (lane == 0) out[r] = bc;
  }
};

__global__ __launch_bounds__(kBlock) void list_minmax_kernel(MinMax f) { for_wave_tiles(f.n, kWave, f); }

// ---- quadratic kernels: set functions and sort in LDS -------------------------------
// Rows of at most kListShort elements (both sides together) compare straight from memory, one lane per
// row; longer rows are staged by the wave in its slice of LDS: 2 sides x kListFastMax x (8 B key + 1 B
// validity) x 4 waves = 36 KB per block.
constexpr int kListShort = 16;

// this wave's LDS writes are visible to all of its lanes
__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

struct SideView {       // one list's keys: child rows in memory, or staged in LDS
  const int64_t* k;
  const uint8_t* v;     // null = all valid (memory view only)
  int64_t base, limit;  // memory view: element i is child row base + i (< limit); LDS view: base 0
  int len;
  __device__ bool val(int i) const { return base + i < limit && (!v || v[base + i]); }
  __device__ int64_t key(int i) const { return k[base + i]; }
  __device__ bool has(int upto, int64_t kk, bool vv) const {
    for (int j = 0; j < upto; ++j) {
      const bool ev = val(j);
      if (vv ? (ev && key(j) == kk) : !ev) return true;
    }
    return false;
  }
};

__device__ inline bool set_keep_a(const SideView& A, const SideView& B, int op, int i) {
  const bool v = A.val(i);
  const int64_t k = v ? A.key(i) : 0;
  if (A.has(i, k, v)) return false;
  if (op == 2) return B.has(B.len, k, v);
  if (op == 3) return !B.has(B.len, k, v);
  return true;
}
__device__ inline bool set_keep_b(const SideView& A, const SideView& B, int j) {
  const bool v = B.val(j);
  const int64_t k = v ? B.key(j) : 0;
  return !A.has(A.len, k, v) && !B.has(j, k, v);
}
__device__ inline bool set_in_a(const SideView& A, const SideView& B, int j) {
  const bool v = B.val(j);
  return A.has(A.len, v ? B.key(j) : 0, v);
}

struct SetOp {
  const int64_t* seA;
  const uint8_t* validA;
  const int64_t* keysA;
  const uint8_t* kvalidA;
  int64_t childA_n;
  const int64_t* seB;      // null for distinct
  const uint8_t* validB;
  const int64_t* keysB;
  const uint8_t* kvalidB;
  int64_t childB_n;
  int op;
  int64_t n;
  const int64_t* offs;     // null: the count pass
  int64_t b_base;
  int64_t cap;             // write pass: elements of out
  int64_t* out;
  int64_t* lds_k;          // this wave's 2 x kListFastMax keys
  uint8_t* lds_v;          // this wave's 2 x kListFastMax validity bytes

  __device__ void sides(int64_t r, SideView& A, SideView& B) const {
    int64_t st, ln;
    row_range(seA, validA, r, st, ln);
    A = SideView{keysA, kvalidA, st, childA_n, (int)(ln < kListFastMax ? ln : kListFastMax)};
    B = SideView{keysB, kvalidB, 0, childB_n, 0};
    if (seB) {
      row_range(seB, validB, r, st, ln);
      B.base = st;
      B.len = (int)(ln < kListFastMax ? ln : kListFastMax);
    }
  }
  __device__ int64_t work(int64_t r) const {
    SideView A, B;
    sides(r, A, B);
    return A.len + B.len;
  }
  __device__ int64_t row_a(const SideView& A, int i) const { return A.base + i < childA_n ? A.base + i : -1; }
  __device__ int64_t row_b(const SideView& B, int j) const {
    return B.base + j < childB_n ? b_base + B.base + j : -1;
  }
  __device__ void short_row(int64_t r) const {
    SideView A, B;
    sides(r, A, B);
    if (op >= 4) {
      bool all = true, any = false;
      for (int j = 0; j < B.len; ++j) {
        const bool in = set_in_a(A, B, j);
        all &= in;
        any |= in;
      }
      out[r] = op == 4 ? all : any;
      return;
    }
    int64_t m = 0, o = offs ? offs[r] : 0;
    for (int i = 0; i < A.len; ++i)
      if (set_keep_a(A, B, op, i)) {
        if (offs) put(out, cap, o + m, row_a(A, i));
        ++m;
      }
    if (op == 1)
      for (int j = 0; j < B.len; ++j)
        if (set_keep_b(A, B, j)) {
          if (offs) put(out, cap, o + m, row_b(B, j));
          ++m;
        }
    if (!offs) out[r] = m;
  }
  __device__ void stage(const SideView& G, int side, int lane, SideView& S) const {
    int64_t* k = lds_k + side * kListFastMax;
    uint8_t* v = lds_v + side * kListFastMax;
    for (int i = lane; i < G.len; i += kWave) {
      const bool ev = G.val(i);
      v[i] = ev;
      k[i] = ev ? G.key(i) : 0;
    }
    S = SideView{k, v, 0, kListFastMax, G.len};
  }
  __device__ void long_row(int64_t r, int lane) const {
    SideView GA, GB, A, B;
    sides(r, GA, GB);
    wave_lds_sync();        // the previous row's readers are done with the buffers
    stage(GA, 0, lane, A);
    stage(GB, 1, lane, B);
    wave_lds_sync();
    if (op >= 4) {
      bool all = true, any = false;
      for (int j = lane; j < B.len; j += kWave) {
        const bool in = set_in_a(A, B, j);
        all &= in;
        any |= in;
      }
      const bool res = op == 4 ? __ballot(!all) == 0 : __ballot(any) != 0;
      if (lane == 0) out[r] = res;
      return;
    }
    const int64_t o = offs ? offs[r] : 0;
    int64_t run = 0;
    for (int base = 0; base < A.len; base += kWave) {
      const int i = base + lane;
      const bool keep = i < A.len && set_keep_a(A, B, op, i);
      const uint64_t kb = __ballot(keep);
      if (offs && keep) put(out, cap, o + run + lane_prefix(kb), row_a(GA, i));
      run += __popcll(kb);
    }
    if (op == 1)
      for (int base = 0; base < B.len; base += kWave) {
        const int j = base + lane;
        const bool keep = j < B.len && set_keep_b(A, B, j);
        const uint64_t kb = __ballot(keep);
        if (offs && keep) put(out, cap, o + run + lane_prefix(kb), row_b(GB, j));
        run += __popcll(kb);
      }
    if (!offs && lane == 0) out[r] = run;
  }
};

__global__ __launch_bounds__(kBlock) void list_set_kernel(SetOp f) {
  __shared__ int64_t lds_k[kWavesPerBlock][2 * kListFastMax];
  __shared__ uint8_t lds_v[kWavesPerBlock][2 * kListFastMax];
  const int w = threadIdx.x / kWave;
  f.lds_k = lds_k[w];
  f.lds_v = lds_v[w];
  for_wave_tiles(f.n, kListShort, f);
}

// array_sort. Elements order by (class, key, position): class 0 NULLs first, 1 values, 2 NULLs last,
// 3 padding up to the power of two the bitonic network needs; descending complements the key.
struct SortOp {
  const int64_t* se;
  const uint8_t* valid;
  const int64_t* keys;
  const uint8_t* kvalid;
  int64_t child_n;
  bool desc, nulls_first;
  int64_t n;
  const int64_t* offs;
  int64_t cap;
  int64_t* out;
  int64_t* lds_k;   // order key per slot
  int64_t* lds_t;   // class << 32 | position per slot

  // the row as sorted: what the offsets leave room for, at most kListFastMax elements
  __device__ int64_t range(int64_t r, int64_t& st) const {
    int64_t ln;
    row_range(se, valid, r, st, ln);
    const int64_t room = offs[r + 1] - offs[r];
    if (ln > room) ln = room;
    return ln < kListFastMax ? ln : kListFastMax;
  }
  __device__ int64_t work(int64_t r) const {
    int64_t st;
    return range(r, st);
  }
  __device__ void elem(int64_t st, int t, int64_t& k, int64_t& tag) const {
    const int64_t c = st + t;
    const bool ev = c < child_n && (!kvalid || kvalid[c]);
    k = ev ? (desc ? ~keys[c] : keys[c]) : 0;
    tag = ((int64_t)(ev ? 1 : (nulls_first ? 0 : 2)) << 32) | t;
  }
  __device__ static bool less(int64_t ka, int64_t ta, int64_t kb, int64_t tb) {
    const int64_t ca = ta >> 32, cb = tb >> 32;
    if (ca != cb) return ca < cb;
    if (ka != kb) return ka < kb;
    return ta < tb;
  }
  __device__ void short_row(int64_t r) const {
    int64_t st;
    const int ln = (int)range(r, st);
    const int64_t o = offs[r];
    for (int i = 0; i < ln; ++i) {   // rank sort: the order is total, so ranks are a permutation
      int64_t ki, ti, kj, tj;
      elem(st, i, ki, ti);
      int rank = 0;
      for (int j = 0; j < ln; ++j) {
        elem(st, j, kj, tj);
        rank += less(kj, tj, ki, ti);
      }
      put(out, cap, o + rank, st + i < child_n ? st + i : -1);
    }
  }
  __device__ void long_row(int64_t r, int lane) const {
    int64_t st;
    const int ln = (int)range(r, st);
    const int64_t o = offs[r];
    int p = kWave;
    while (p < ln) p <<= 1;
    wave_lds_sync();
    for (int i = lane; i < p; i += kWave) {
      int64_t k = 0, tag = ((int64_t)3 << 32) | i;
      if (i < ln) elem(st, i, k, tag);
      lds_k[i] = k;
      lds_t[i] = tag;
    }
    wave_lds_sync();
    for (int size = 2; size <= p; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = lane; i < p; i += kWave) {
          const int j = i ^ stride;
          if (j > i) {
            const int64_t ki = lds_k[i], ti = lds_t[i], kj = lds_k[j], tj = lds_t[j];
            const bool up = (i & size) == 0;
            if (less(kj, tj, ki, ti) == up) {
              lds_k[i] = kj;
              lds_t[i] = tj;
              lds_k[j] = ki;
              lds_t[j] = ti;
            }
          }
        }
        wave_lds_sync();
      }
    for (int i = lane; i < ln; i += kWave) {
      const int64_t c = st + (lds_t[i] & 0xffffffffLL);
      put(out, cap, o + i, c < child_n ? c : -1);
    }
  }
};

__global__ __launch_bounds__(kBlock) void list_sort_kernel(SortOp f) {
  __shared__ int64_t lds[kWavesPerBlock][2 * kListFastMax];
  const int w = threadIdx.x / kWave;
  f.lds_k = lds[w];
  f.lds_t = lds[w] + kListFastMax;
  for_wave_tiles(f.n, kListShort, f);
}

// ---- map lookup ----------------------------------------------------------------------
// m[k] / element_at / map_extract: the child row of the first entry of the row whose key equals
// the needle, -1 for none (no match, NULL map row, NULL needle, malformed slot). Keys are read
// where they lie: fixed-width keys at their native width against an int64 needle, plain UTF-8
// keys by length first and bytes after. Rows of at most a wave's width run one lane per row;
// longer rows are strided by the wave and the lowest matching lane of the first matching stride
// wins, so duplicate keys (imported, unvalidated maps) resolve to the first entry.
template <class K>
struct FixedKeys {
  const K* keys;
  const uint8_t* kvalid;
  const int64_t* needle;        // per row, or null: needle_const
  const uint8_t* needle_valid;
  int64_t needle_const;
  using Needle = int64_t;
  __device__ bool load(int64_t r, Needle& nd) const {
    if (!needle) {
      nd = needle_const;
      return true;
    }
    nd = needle[r];
    return row_ok(needle_valid, r);
  }
  __device__ bool hit(int64_t c, const Needle& nd) const { return (!kvalid || kvalid[c]) && (int64_t)keys[c] == nd; }
};

// len bytes at a and b are equal: dwords where both pointers reach 4-byte alignment together
// (entries start at arbitrary byte offsets), bytes for the head, the tail and everything else
__device__ inline bool bytes_equal(const uint8_t* a, const uint8_t* b, int64_t len) {
  int64_t i = 0;
  if ((((uintptr_t)a ^ (uintptr_t)b) & 3) == 0) {
    for (; i < len && (((uintptr_t)(a + i)) & 3); ++i)
      if (a[i] != b[i]) return false;
    for (; i + 4 <= len; i += 4)
      if (*reinterpret_cast<const uint32_t*>(a + i) != *reinterpret_cast<const uint32_t*>(b + i)) return false;
  }
  for (; i < len; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

struct StringKeys {
  const int64_t* offs;          // child_n + 1
  const uint8_t* bytes;
  int64_t nbytes;
  const uint8_t* kvalid;
  const int64_t* needle_offs;   // per row (n + 1), or null: a constant
  const uint8_t* needle_bytes;  // constant: 4 copies, copy m at m * const_stride + m (address = m mod 4)
  int64_t needle_nbytes;
  const uint8_t* needle_valid;
  int64_t const_len, const_stride;
  struct Needle {
    const uint8_t* p;
    int64_t len;
  };
  __device__ bool load(int64_t r, Needle& nd) const {
    if (!needle_offs) {
      nd = Needle{needle_bytes, const_len};
      return true;
    }
    const int64_t a = needle_offs[r], b = needle_offs[r + 1];
    nd = Needle{needle_bytes + a, b - a};
    return row_ok(needle_valid, r) && a >= 0 && b >= a && b <= needle_nbytes;
  }
  __device__ bool hit(int64_t c, const Needle& nd) const {
    if (kvalid && !kvalid[c]) return false;
    const int64_t a = offs[c], b = offs[c + 1];
    if (b - a != nd.len || a < 0 || b > nbytes) return false;
    const uint8_t* k = bytes + a;
    const uint8_t* q = nd.p;
    if (!needle_offs) {           // the copy that shares this key's alignment: dword compares throughout
      const int64_t m = (int64_t)((uintptr_t)k & 3);
      q += m * const_stride + m;
    }
    return bytes_equal(k, q, nd.len);
  }
};

template <class Keys>
struct MapLookup {
  const int64_t* se;
  const uint8_t* valid;
  int64_t n, child_n;
  Keys keys;
  int64_t* out;
  // entries of the row that lie inside the child
  __device__ void range(int64_t r, int64_t& st, int64_t& ln) const {
    row_range(se, valid, r, st, ln);
    if (st >= child_n) ln = 0;
    else if (ln > child_n - st) ln = child_n - st;
  }
  __device__ int64_t work(int64_t r) const {
    int64_t st, ln;
    range(r, st, ln);
    return ln;
  }
  __device__ void short_row(int64_t r) const {
    int64_t st, ln, res = -1;
    range(r, st, ln);
    typename Keys::Needle nd;
    if (keys.load(r, nd))
      for (int64_t t = 0; t < ln; ++t)
        if (keys.hit(st + t, nd)) {
          res = st + t;
          break;
        }
    out[r] = res;
  }
  __device__ void long_row(int64_t r, int lane) const {
    int64_t st, ln, res = -1;
    range(r, st, ln);
    typename Keys::Needle nd;
    const bool ok = keys.load(r, nd);   // wave-uniform: one row
    for (int64_t base = 0; ok && base < ln && res < 0; base += kWave) {
      const int64_t t = base + lane;
      const uint64_t hb = __ballot(t < ln && keys.hit(st + t, nd));
      if (hb) res = st + base + __ffsll((unsigned long long)hb) - 1;
    }
    if (lane == 0) out[r] = res;
  }
};

template <class Keys>
__global__ __launch_bounds__(kBlock) void map_lookup_kernel(MapLookup<Keys> f) { for_wave_tiles(f.n, kWave, f); }

inline unsigned tile_grid(int64_t n) { return grid_for(n, kBlock, 1 << 16); }

}  // namespace

void list_slice_se(const int64_t* se, const uint8_t* valid, const int64_t* from, const uint8_t* from_valid,
                   const int64_t* to, const uint8_t* to_valid, int64_t from_const, int64_t to_const, int64_t n,
                   int64_t* out_se, uint8_t* out_valid, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(list_slice_se_kernel, dim3(tile_grid(n)), dim3(kBlock), 0, s, se, valid, from, from_valid, to,
                     to_valid, from_const, to_const, n, out_se, out_valid);
  check_launch("list_slice_se", s);
}

void list_parts_count(const int64_t* parts, int k, int64_t n, int64_t* out_len, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(list_parts_count_kernel, dim3(tile_grid(n)), dim3(kBlock), 0, s, parts, k, n, out_len);
  check_launch("list_parts_count", s);
}

void list_parts_write(const int64_t* parts, int k, int64_t n, const int64_t* offs, int64_t src_n, int64_t cap,
                      int64_t* idx, int64_t* out_se, hipStream_t s) {
  if (n == 0) return;
  PartsWrite f{parts, k, n, offs, src_n, cap, idx, out_se};
  hipLaunchKernelGGL(list_parts_write_kernel, dim3(tile_grid(n)), dim3(kBlock), 0, s, f);
  check_launch("list_parts_write", s);
}

void list_flatten_count(const int64_t* se, const uint8_t* valid, const int64_t* ise, const uint8_t* ivalid,
                        int64_t n, int64_t inner_n, int64_t* out_len, hipStream_t s) {
  if (n == 0) return;
  Flatten f{se, valid, ise, ivalid, n, inner_n, nullptr, 0, 0, out_len, nullptr};
  hipLaunchKernelGGL(list_flatten_kernel, dim3(tile_grid(n)), dim3(kBlock), 0, s, f);
  check_launch("list_flatten_count", s);
}

void list_flatten_write(const int64_t* se, const uint8_t* valid, const int64_t* ise, const uint8_t* ivalid,
                        int64_t n, int64_t inner_n, const int64_t* offs, int64_t child_n, int64_t cap,
                        int64_t* idx, int64_t* out_se, hipStream_t s) {
  if (n == 0) return;
  Flatten f{se, valid, ise, ivalid, n, inner_n, offs, child_n, cap, idx, out_se};
  hipLaunchKernelGGL(list_flatten_kernel, dim3(tile_grid(n)), dim3(kBlock), 0, s, f);
  check_launch("list_flatten_write", s);
}

void list_match_count(const int64_t* se, const uint8_t* valid, const int64_t* keys, const uint8_t* kvalid,
                      int64_t child_n, const int64_t* needle, const uint8_t* needle_valid, const int64_t* from,
                      const int64_t* limit, int64_t limit_const, int mode, int64_t n, int64_t* out, hipStream_t s) {
  if (n == 0) return;
  if (mode < 0 || mode > 2) throw std::invalid_argument("list_match_count: mode");
  Match f{se,    valid,       keys, kvalid, child_n, needle, needle_valid, from,
          limit, limit_const, mode, n,      nullptr, 0,      0,            out};
  hipLaunchKernelGGL(list_match_kernel, dim3(tile_grid(n)), dim3(kBlock), 0, s, f);
  check_launch("list_match_count", s);
}

void list_match_write(const int64_t* se, const uint8_t* valid, const int64_t* keys, const uint8_t* kvalid,
                      int64_t child_n, const int64_t* needle, const uint8_t* needle_valid, const int64_t* limit,
                      int64_t limit_const, int mode, int64_t n, const int64_t* offs, int64_t repl_base,
                      int64_t cap, int64_t* out, hipStream_t s) {
  if (n == 0) return;
  if (mode < 0 || mode > 2) throw std::invalid_argument("list_match_write: mode");
  Match f{se,    valid,       keys,      kvalid, child_n, needle,    needle_valid, nullptr,
          limit, limit_const, 10 + mode, n,      offs,    repl_base, cap,          out};
  hipLaunchKernelGGL(list_match_kernel, dim3(tile_grid(n)), dim3(kBlock), 0, s, f);
  check_launch("list_match_write", s);
}

void list_minmax_idx(const int64_t* se, const uint8_t* valid, const int64_t* keys, const uint8_t* kvalid,
                     int64_t child_n, int is_max, int64_t n, int64_t* out, hipStream_t s) {
  if (n == 0) return;
  MinMax f{se, valid, keys, kvalid, child_n, is_max != 0, n, out};
  hipLaunchKernelGGL(list_minmax_kernel, dim3(tile_grid(n)), dim3(kBlock), 0, s, f);
  check_launch("list_minmax_idx", s);
}

void list_set_count(const int64_t* seA, const uint8_t* validA, const int64_t* keysA, const uint8_t* kvalidA,
                    int64_t childA_n, const int64_t* seB, const uint8_t* validB, const int64_t* keysB,
                    const uint8_t* kvalidB, int64_t childB_n, int op, int64_t n, int64_t* out, hipStream_t s) {
  if (n == 0) return;
  if (op < 0 || op > 5 || (op > 0 && !seB)) throw std::invalid_argument("list_set_count: op");
  SetOp f{seA, validA, keysA, kvalidA, childA_n, seB, validB, keysB, kvalidB, childB_n, op, n, nullptr, 0, 0, out,
          nullptr, nullptr};
  hipLaunchKernelGGL(list_set_kernel, dim3(tile_grid(n)), dim3(kBlock), 0, s, f);
  check_launch("list_set_count", s);
}

void list_set_write(const int64_t* seA, const uint8_t* validA, const int64_t* keysA, const uint8_t* kvalidA,
                    int64_t childA_n, const int64_t* seB, const uint8_t* validB, const int64_t* keysB,
                    const uint8_t* kvalidB, int64_t childB_n, int op, int64_t n, const int64_t* offs,
                    int64_t b_base, int64_t cap, int64_t* idx, hipStream_t s) {
  if (n == 0) return;
  if (op < 0 || op > 3 || (op > 0 && !seB)) throw std::invalid_argument("list_set_write: op");
  SetOp f{seA, validA, keysA, kvalidA, childA_n, seB, validB, keysB, kvalidB, childB_n, op, n, offs, b_base, cap, idx,
          nullptr, nullptr};
  hipLaunchKernelGGL(list_set_kernel, dim3(tile_grid(n)), dim3(kBlock), 0, s, f);
  check_launch("list_set_write", s);
}

void list_sort_idx(const int64_t* se, const uint8_t* valid, const int64_t* keys, const uint8_t* kvalid,
                   int64_t child_n, int desc, int nulls_first, int64_t n, const int64_t* offs, int64_t cap,
                   int64_t* idx, hipStream_t s) {
  if (n == 0) return;
  SortOp f{se, valid, keys, kvalid, child_n, desc != 0, nulls_first != 0, n, offs, cap, idx, nullptr, nullptr};
  hipLaunchKernelGGL(list_sort_kernel, dim3(tile_grid(n)), dim3(kBlock), 0, s, f);
  check_launch("list_sort_idx", s);
}

template <class K>
static void map_lookup_fixed(const int64_t* se, const uint8_t* valid, int64_t n, int64_t child_n, const void* keys,
                             const uint8_t* kvalid, const int64_t* needle, const uint8_t* needle_valid,
                             int64_t needle_const, int64_t* out, hipStream_t s) {
  MapLookup<FixedKeys<K>> f{se, valid, n, child_n,
                            FixedKeys<K>{static_cast<const K*>(keys), kvalid, needle, needle_valid, needle_const}, out};
  hipLaunchKernelGGL(map_lookup_kernel<FixedKeys<K>>, dim3(tile_grid(n)), dim3(kBlock), 0, s, f);
}

void map_lookup_idx(const int64_t* se, const uint8_t* valid, int64_t n, int64_t child_n, int key_width,
                    const void* keys, const uint8_t* kvalid, const int64_t* needle, const uint8_t* needle_valid,
                    int64_t needle_const, int64_t* out, hipStream_t s) {
  if (n == 0) return;
  switch (key_width) {
    case 1: map_lookup_fixed<int8_t>(se, valid, n, child_n, keys, kvalid, needle, needle_valid, needle_const, out, s); break;
    case 2: map_lookup_fixed<int16_t>(se, valid, n, child_n, keys, kvalid, needle, needle_valid, needle_const, out, s); break;
    case 4: map_lookup_fixed<int32_t>(se, valid, n, child_n, keys, kvalid, needle, needle_valid, needle_const, out, s); break;
    case 8: map_lookup_fixed<int64_t>(se, valid, n, child_n, keys, kvalid, needle, needle_valid, needle_const, out, s); break;
    default: throw std::invalid_argument("map_lookup_idx: key width");
  }
  check_launch("map_lookup_idx", s);
}

void map_lookup_idx_str(const int64_t* se, const uint8_t* valid, int64_t n, int64_t child_n, const int64_t* key_offs,
                        const uint8_t* key_bytes, int64_t key_nbytes, const uint8_t* kvalid,
                        const int64_t* needle_offs, const uint8_t* needle_bytes, int64_t needle_nbytes,
                        const uint8_t* needle_valid, int64_t const_len, int64_t const_stride, int64_t* out,
                        hipStream_t s) {
  if (n == 0) return;
  if (!needle_offs && (const_len < 0 || const_stride < const_len || (const_stride & 3) ||
                       needle_nbytes < 4 * const_stride + 3 || ((uintptr_t)needle_bytes & 3)))
    throw std::invalid_argument("map_lookup_idx_str: constant needle buffer");
  MapLookup<StringKeys> f{se, valid, n, child_n,
                          StringKeys{key_offs, key_bytes, key_nbytes, kvalid, needle_offs, needle_bytes, needle_nbytes,
                                     needle_valid, const_len, const_stride},
                          out};
  hipLaunchKernelGGL(map_lookup_kernel<StringKeys>, dim3(tile_grid(n)), dim3(kBlock), 0, s, f);
  check_launch("map_lookup_idx", s);
}

void list_element_idx(const int64_t* se, const uint8_t* valid, const int64_t* pos, const uint8_t* pos_valid,
                      int64_t pos_const, int64_t n, int64_t child_n, int64_t* out, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(list_element_idx_kernel, dim3(grid_for(n, kBlock, 1 << 16)), dim3(kBlock), 0, s, se, valid, pos,
                     pos_valid, pos_const, n, child_n, out);
  check_launch("list_element_idx", s);
}

void interleave_idx(int64_t n, int k, int64_t* out, hipStream_t s) {
  if (n == 0 || k == 0) return;
  hipLaunchKernelGGL(interleave_idx_kernel, dim3(grid_for(n * k, kBlock, 1 << 16)), dim3(kBlock), 0, s, n, k, out);
  check_launch("interleave_idx", s);
}

void list_slots(int64_t n, int64_t k, int64_t* se, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(list_slots_kernel, dim3(grid_for(n, kBlock, 1 << 16)), dim3(kBlock), 0, s, n, k, se);
  check_launch("list_slots", s);
}

}  // namespace kern
}  // namespace igloo
