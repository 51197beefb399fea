// pybind11 module `igloo_amd._native`: SQL parser + gfx950 kernel launchers +
// device runtime. Pointer arguments are passed as integers (torch
// tensor.data_ptr()); shape/dtype validation happens in igloo_amd/ops before
// any launch, so this layer is a thin, allocation-free trampoline.
// A launcher that needs nothing but those casts is bound as raw<&kern::name>:
// the adaptor deduces the signature from kernels.h, takes uintptr_t for every
// pointer (hipStream_t included) and casts it back to the launcher's own type.
// Bindings that check, build an argument or release the GIL stay lambdas.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <tuple>
#include <memory>
#include <vector>

#include "io/parquet_meta.h"
#include "kernels/kernels.h"
#include "runtime/runtime.h"
#include "sql/ast.h"
#include "sql/ast_py.h"

namespace py = pybind11;
using namespace igloo;

namespace {

template <typename T>
T* P(uintptr_t p) {
  return reinterpret_cast<T*>(p);
}
hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

// raw<&f>: f with each pointer parameter taken as uintptr_t; all else unchanged (a bound struct such
// as kern::JoinTableRef, taken by const reference, passes through as that reference)
template <typename T>
struct py_arg {
  using type = T;
  static T get(T v) { return v; }
};
template <typename T>
struct py_arg<T*> {
  using type = uintptr_t;
  static T* get(uintptr_t v) { return reinterpret_cast<T*>(v); }
};
template <auto F>
struct raw_t;
template <typename R, typename... A, R (*F)(A...)>
struct raw_t<F> {
  R operator()(typename py_arg<A>::type... a) const { return F(py_arg<A>::get(a)...); }
};
template <auto F>
constexpr raw_t<F> raw{};

// the (op, src64, src, valid, dst, dst2) list of the aggregate bindings
using AggDescArg = std::vector<std::tuple<int, int, uintptr_t, uintptr_t, uintptr_t, uintptr_t>>;
std::vector<kern::AggDesc> agg_descs(const AggDescArg& descs) {
  std::vector<kern::AggDesc> d;
  for (auto& t : descs)
    d.push_back({std::get<0>(t), std::get<1>(t), P<const void>(std::get<2>(t)), P<const uint8_t>(std::get<3>(t)),
                 P<void>(std::get<4>(t)), P<void>(std::get<5>(t))});
  return d;
}

py::list parse(const std::string& text) {
  py::list out;
  try {
    for (auto& st : sql::parse_sql(text)) out.append(sql::to_python(st));
  } catch (const sql::ParseError& e) {
    PyErr_SetString(PyExc_SyntaxError, e.what());
    throw py::error_already_set();
  }
  return out;
}

py::list tokenize(const std::string& text) {
  py::list out;
  static const char* names[] = {"ident", "quoted_ident", "keyword", "number", "string", "op", "end"};
  try {
    for (auto& t : sql::tokenize(text)) out.append(py::make_tuple(names[t.kind], t.text, t.pos));
  } catch (const sql::ParseError& e) {
    PyErr_SetString(PyExc_SyntaxError, e.what());
    throw py::error_already_set();
  }
  return out;
}

py::dict leaf_dict(const io::PqLeaf& l) {
  py::dict d;
  d["name"] = l.name;
  d["type"] = l.type;
  d["type_length"] = l.type_length;
  d["max_def"] = l.max_def;
  d["max_rep"] = l.max_rep;
  d["converted_type"] = l.converted_type;
  d["logical"] = l.logical;
  d["tz"] = l.tz;
  d["scale"] = l.scale;
  d["precision"] = l.precision;
  d["top"] = l.top;
  d["kind"] = l.kind;
  d["rep_def"] = l.rep_def;
  d["anc_def"] = l.anc_def;
  return d;
}

py::dict chunk_dict(const io::PqChunk& c) {
  py::dict d;
  d["type"] = c.type;
  d["codec"] = c.codec;
  d["num_values"] = c.num_values;
  d["start"] = c.start();
  d["length"] = c.total_compressed;
  d["uncompressed"] = c.total_uncompressed;
  d["data_page_offset"] = c.data_page_offset;
  d["dictionary_page_offset"] = c.dictionary_page_offset;
  d["encodings"] = c.encodings;
  d["external"] = c.external;
  d["null_count"] = c.stats.has_nulls ? py::object(py::int_(c.stats.null_count)) : py::object(py::none());
  d["min"] = c.stats.has_min ? py::object(py::bytes(c.stats.min)) : py::object(py::none());
  d["max"] = c.stats.has_max ? py::object(py::bytes(c.stats.max)) : py::object(py::none());
  return d;
}

py::dict page_header_dict(const io::PqPageHeader& h) {
  py::dict d;
  d["type"] = h.type;
  d["header_len"] = h.header_len;
  d["compressed"] = h.compressed;
  d["uncompressed"] = h.uncompressed;
  d["num_values"] = h.num_values;
  d["encoding"] = h.encoding;
  d["def_encoding"] = h.def_encoding;
  d["num_nulls"] = h.num_nulls;
  d["num_rows"] = h.num_rows;
  d["def_len"] = h.def_len;
  d["rep_len"] = h.rep_len;
  d["is_compressed"] = h.is_compressed;
  return d;
}

kern::PqDecodeSpec decode_spec(const py::dict& d, bool need_output = true) {
  kern::PqDecodeSpec s{};
  s.phys = d["phys"].cast<int>();
  s.type_len = d["type_len"].cast<int>();
  s.out_width = d["out_width"].cast<int>();
  s.conv = d["conv"].cast<int>();
  s.conv_k = d["conv_k"].cast<int64_t>();
  s.max_def = d["max_def"].cast<int>();
  s.max_rep = d.contains("max_rep") ? d["max_rep"].cast<int>() : 0;
  s.out = P<void>(d["out"].cast<uintptr_t>());
  s.valid = P<uint8_t>(d["valid"].cast<uintptr_t>());
  s.scratch = P<uint32_t>(d["scratch"].cast<uintptr_t>());
  s.str_len = P<int64_t>(d["str_len"].cast<uintptr_t>());
  s.str_pos = P<int64_t>(d["str_pos"].cast<uintptr_t>());
  s.codes = P<int32_t>(d["codes"].cast<uintptr_t>());
  s.dict_len = P<int64_t>(d["dict_len"].cast<uintptr_t>());
  s.dict_pos = P<int64_t>(d["dict_pos"].cast<uintptr_t>());
  s.raw = P<const uint8_t>(d["raw"].cast<uintptr_t>());
  s.dec = P<const uint8_t>(d["dec"].cast<uintptr_t>());
  s.error = P<int>(d["error"].cast<uintptr_t>());
  if (s.max_def < 0 || s.max_def > 3 || s.max_rep < 0 || s.max_rep > 1 || s.phys < 0 || s.phys > kern::PQ_PHYS_FLBA || !s.raw || !s.error)
    throw std::runtime_error("pq_decode: bad spec");
  if (need_output && (s.phys == kern::PQ_PHYS_BYTE_ARRAY ? !(s.codes || (s.str_len && s.str_pos)) : !s.out))
    throw std::runtime_error("pq_decode: missing output buffer");
  return s;
}

}  // namespace

namespace igloo {
void register_jit(py::module_& m);  // runtime/jit.cpp
void register_arrow_device(py::module_& m);  // runtime/arrow_device.cpp
}

PYBIND11_MODULE(_native, m) {
  m.doc() = "igloo MI355X native core: SQL frontend, gfx950 kernels, device runtime";
  m.attr("ARCH") = "gfx950";
  m.attr("MAX_AGGS") = kern::kMaxAggs;
  m.attr("MAX_GATHER_COLS") = kern::kMaxGatherCols;
  m.attr("MAX_PARTS") = kern::kMaxParts;
  igloo::register_jit(m);
  igloo::register_arrow_device(m);

  // ------------------------------------------------------------------ SQL
  m.def("parse_sql", &parse, "Parse SQL text into a list of statement ASTs (dicts)");
  m.def("tokenize", &tokenize);

  // -------------------------------------------------------------- runtime
  m.def("device_count", &rt::device_count);
  m.def("device_info", [](int dev) {
    auto d = rt::device_info(dev);
    py::dict r;
    r["device"] = d.device;
    r["name"] = d.name;
    r["arch"] = d.arch;
    r["total_mem"] = d.total_mem;
    r["free_mem"] = d.free_mem;
    r["cu_count"] = d.cu_count;
    r["wave_size"] = d.wave_size;
    r["lds_per_block"] = d.lds_per_block;
    r["l2_bytes"] = d.l2_bytes;
    r["clock_khz"] = d.clock_khz;
    return r;
  });
  py::class_<rt::PinnedPool>(m, "PinnedPool")
      .def(py::init<size_t>())
      .def("acquire",
           [](rt::PinnedPool& p, size_t bytes) {
             size_t got = 0;
             void* ptr = p.acquire(bytes, &got);
             return py::make_tuple((uintptr_t)ptr, got);
           })
      .def("release", [](rt::PinnedPool& p, uintptr_t ptr, size_t bytes) { p.release((void*)ptr, bytes); })
      .def_property_readonly("cached_bytes", &rt::PinnedPool::cached_bytes);

  // ------------------------------------------------------- select / scan
  m.def("select_num_tiles", &kern::select_num_tiles);
  m.def("select_count", raw<&kern::select_count>);
  // tile counts a fused scan wrote with its mask -> exclusive offsets in place + total
  m.def("select_scan_counts", [](uintptr_t counts, int64_t tiles, uintptr_t total, uintptr_t s) {
    if (!counts || !total || tiles <= 0) throw std::runtime_error("select_scan_counts: bad arguments");
    kern::scan_counts(P<int64_t>(counts), tiles, P<int64_t>(total), S(s));
  });
  m.def("select_write", raw<&kern::select_write>);
  m.def("select_compact", [](uintptr_t mask, int64_t n, uintptr_t tiles,
                             const std::vector<std::tuple<uintptr_t, uintptr_t, int, uintptr_t, uintptr_t>>& cols,
                             uintptr_t idx, bool idx64, int64_t cap, uintptr_t s) {
    kern::CompactArgs a{};
    if ((int)cols.size() > kern::kMaxCompactCols) throw std::runtime_error("select_compact: too many columns");
    for (size_t j = 0; j < cols.size(); ++j) {
      auto& c = cols[j];
      a.cols[j] = {P<void>(std::get<0>(c)), P<void>(std::get<1>(c)), std::get<2>(c), P<uint8_t>(std::get<3>(c)),
                   P<uint8_t>(std::get<4>(c))};
    }
    a.ncols = (int)cols.size();
    a.idx = P<void>(idx);
    a.idx64 = idx64;
    kern::select_compact(P<uint8_t>(mask), n, P<int64_t>(tiles), a, cap, S(s));
  });
  m.def("scan_workspace_tiles", &kern::scan_workspace_tiles);
  m.def("exclusive_scan", raw<&kern::exclusive_scan>);
  // ---- pack.hip
  auto pack_spec = [](const std::vector<std::tuple<uintptr_t, uintptr_t, int, int>>& cols, int row_bytes) {
    if (cols.size() > (size_t)kern::kMaxPackCols) throw std::runtime_error("pack: too many columns");
    kern::PackSpec spec{};
    spec.ncols = (int32_t)cols.size();
    spec.row_bytes = row_bytes;
    for (size_t i = 0; i < cols.size(); ++i) {
      spec.cols[i].src = P<const void>(std::get<0>(cols[i]));
      spec.cols[i].dst = P<void>(std::get<1>(cols[i]));
      spec.cols[i].width = std::get<2>(cols[i]);
      spec.cols[i].offset = std::get<3>(cols[i]);
      if (spec.cols[i].offset + spec.cols[i].width > row_bytes) throw std::runtime_error("pack: field outside row");
    }
    return spec;
  };
  m.def("pack_rows", [pack_spec](std::vector<std::tuple<uintptr_t, uintptr_t, int, int>> cols, int row_bytes,
                                 uintptr_t perm, bool perm64, int64_t n, uintptr_t out, uintptr_t s) {
    kern::pack_rows(pack_spec(cols, row_bytes), P<const void>(perm), perm64, n, P<uint8_t>(out), S(s));
  });
  m.def("unpack_rows", [pack_spec](std::vector<std::tuple<uintptr_t, uintptr_t, int, int>> cols, int row_bytes,
                                   uintptr_t in, int64_t n, uintptr_t s) {
    kern::unpack_rows(pack_spec(cols, row_bytes), P<const uint8_t>(in), n, S(s));
  });
  // ---- util.hip
  m.def("column_stats", raw<&kern::column_stats>);
  m.def("run_bounds", raw<&kern::run_bounds>);
  m.def("mark_slot_rows", raw<&kern::mark_slot_rows>);
  m.def("pack_bits", [](std::vector<uintptr_t> cols, std::vector<bool> is64, std::vector<int64_t> lo,
                        std::vector<int> shift, int64_t n, uintptr_t out, uintptr_t s) {
    std::vector<const void*> c(cols.size());
    std::unique_ptr<bool[]> w(new bool[cols.size()]);
    for (size_t i = 0; i < cols.size(); ++i) {
      c[i] = reinterpret_cast<const void*>(cols[i]);
      w[i] = is64[i];
    }
    kern::pack_bits(c.data(), w.get(), lo.data(), shift.data(), (int)cols.size(), n, P<int64_t>(out), S(s));
  });
  m.def("differs_from_rep", raw<&kern::differs_from_rep>);
  m.def("mark_keys", raw<&kern::mark_keys>);
  m.def("probe_marks", raw<&kern::probe_marks>);
  m.def("const_ints", [](uintptr_t out, std::vector<int64_t> vals, uintptr_t s) {
    kern::const_ints(P<int64_t>(out), vals.data(), (int64_t)vals.size(), S(s));
  });
  m.def("end_capture", raw<&kern::end_capture>);
  m.def("wide_fits", raw<&kern::wide_fits>);
  m.def("avg_wide", raw<&kern::avg_wide>);
  // ---- sort.hip
  m.def("radix_sort_ws_bytes", &kern::radix_sort_ws_bytes);
  m.def("radix_sort_pairs", raw<&kern::radix_sort_pairs>);
  m.def("sort_key_pack", [](std::vector<std::tuple<uintptr_t, uintptr_t, uint64_t, uint64_t, int, int, int, int, int>> cols,
                            uintptr_t perm, bool perm64, int64_t n, uintptr_t out, bool out32, uintptr_t s) {
    if (cols.empty() || cols.size() > (size_t)kern::kMaxSortCols) throw std::runtime_error("sort_key_pack: bad column count");
    kern::SortKeySpec spec{};
    spec.ncols = (int32_t)cols.size();
    int total = 0;
    for (size_t i = 0; i < cols.size(); ++i) {
      auto& c = spec.cols[i];
      const auto& t = cols[i];
      c.ptr = P<const void>(std::get<0>(t));
      c.valid = P<const uint8_t>(std::get<1>(t));
      c.lo = std::get<2>(t);
      c.span = std::get<3>(t);
      c.kind = std::get<4>(t);
      c.width = std::get<5>(t);
      c.bits = std::get<6>(t);
      c.desc = std::get<7>(t);
      c.nulls_first = std::get<8>(t);
      if (c.bits < 0 || c.bits > 64) throw std::runtime_error("sort_key_pack: bad field width");
      total += c.bits + (c.valid ? 1 : 0);
    }
    if (total > (out32 ? 32 : 64)) throw std::runtime_error("sort_key_pack: key fields exceed the key width");
    kern::sort_key_pack(spec, P<const void>(perm), perm64, n, P<void>(out), out32, S(s));
  });
  m.def("radix_digit_hist", raw<&kern::radix_digit_hist>);
  m.def("radix_le_mask", raw<&kern::radix_le_mask>);

  // ------------------------------------------------------------ hash tables
  // A join table and a key column, described once (kernels.h): value classes built from pointers as
  // unsigned integers, like every py_arg<T*>, and handed to the entry points by reference. The
  // table's fields go by name only: positions of the same type cannot be swapped.
  py::class_<kern::JoinTableRef>(m, "JoinTableRef")
      .def(py::init([](uintptr_t tkeys, uintptr_t thead, uintptr_t cstart, uintptr_t crows, bool rid64, int64_t cap,
                       int64_t kmin, bool direct, uintptr_t bits, uint64_t bmask, uintptr_t fold, int64_t n_build) {
             return kern::JoinTableRef{P<int64_t>(tkeys), P<void>(thead), P<void>(cstart), P<void>(crows),
                                       rid64,             cap,            kmin,            direct,
                                       P<uint32_t>(bits), bmask,          P<uint32_t>(fold), n_build};
           }),
           py::kw_only(), py::arg("tkeys"), py::arg("thead"), py::arg("cstart") = 0, py::arg("crows") = 0,
           py::arg("rid64"), py::arg("cap"), py::arg("kmin"), py::arg("direct"), py::arg("bits") = 0,
           py::arg("bmask") = 0, py::arg("fold") = 0, py::arg("n_build"));
  py::class_<kern::KeyColumn>(m, "KeyColumn")
      .def(py::init([](uintptr_t keys, bool key64, uintptr_t valid, int64_t n) {
             return kern::KeyColumn{P<const void>(keys), key64, P<const uint8_t>(valid), n};
           }),
           py::arg("keys"), py::arg("key64"), py::arg("valid"), py::arg("n"));
  m.def("join_build", raw<&kern::join_build>);
  m.def("join_csr_count", raw<&kern::join_csr_count>);
  m.def("join_csr_scatter", raw<&kern::join_csr_scatter>);
  m.def("join_probe", raw<&kern::join_probe>);
  m.def("probe_hit_tiles", &kern::probe_hit_tiles);
  m.def("probe_hits", raw<&kern::probe_hits>);
  m.def("set_probe_grid_cap", &kern::set_probe_grid_cap);
  m.def("set_probe_bits", &kern::set_probe_bits);
  m.def("set_probe_stream_min_rows", &kern::set_probe_stream_min_rows);
  m.def("set_probe_stream_max_fill", &kern::set_probe_stream_max_fill);
  m.def("last_probe_kernel", []() { return std::string(kern::last_probe_kernel()); });
  m.attr("kFoldMinRows") = kern::probe_fold_min_rows();
  m.attr("kFoldWords") = kern::probe_fold_words();
  m.def("probe_fold_needed", &kern::probe_fold_needed);
  m.def("probe_fold_build", [](uintptr_t bits, int64_t cap, uintptr_t fold, uintptr_t s) {
    if (!bits || !fold || cap <= 0) throw std::runtime_error("probe_fold_build: null buffer");
    kern::probe_fold_build(P<const uint32_t>(bits), cap, P<uint32_t>(fold), S(s));
  });
  m.def("join_table_init", [](uintptr_t thead, bool rid64, int64_t cap, uintptr_t tkeys, uintptr_t bits, int64_t nbw,
                              uintptr_t dups, uintptr_t s) {
    if (!thead || !dups || cap <= 0 || (bits && nbw <= 0)) throw std::runtime_error("join_table_init: null buffer");
    kern::join_table_init(P<void>(thead), rid64, cap, P<int64_t>(tkeys), P<uint32_t>(bits), nbw,
                          P<unsigned long long>(dups), S(s));
  });
  m.def("probe_write", raw<&kern::probe_write>);
  m.def("join_expand", raw<&kern::join_expand>);
  // fused scan kernels. cols: [(ptr, width)], terms: [(col, kind, lo, hi, set)],
  // keys: [(col, lo, mul)], aggs: [(op, checked, [(col, a, b)], dst, dst2, shared)]
  using FfCols = std::vector<std::pair<uintptr_t, int64_t>>;
  using FfTerms = std::vector<std::tuple<int, int, int64_t, int64_t, uint64_t>>;
  using FfKeys = std::vector<std::tuple<int, int64_t, int64_t>>;
  using FfAggs = std::vector<std::tuple<int, int, std::vector<std::tuple<int64_t, int64_t, int64_t>>, uintptr_t,
                                        uintptr_t, int, int>>;
  auto make_ff = [](const FfCols& cols, const FfTerms& terms, uintptr_t mask) {
    if (cols.size() > (size_t)kern::kFfMaxCols || terms.size() > (size_t)kern::kFfMaxTerms)
      throw std::runtime_error("fused scan: too many columns / terms");
    kern::FfSpec f{};
    f.ncols = (int32_t)cols.size();
    for (size_t i = 0; i < cols.size(); ++i) {
      f.cols[i].ptr = reinterpret_cast<const void*>(cols[i].first);
      f.cols[i].width = cols[i].second;
      const int64_t w = f.cols[i].width;  // signed 1/2/4/8-byte integer columns
      if (!(w == 1 || w == 2 || w == 4 || w == 8) || (cols[i].first % (w < 4 ? 4 : w)) != 0)
        throw std::runtime_error("fused scan: bad column width / alignment");
    }
    f.nterms = (int32_t)terms.size();
    for (size_t i = 0; i < terms.size(); ++i) {
      auto [col, kind, lo, hi, set] = terms[i];
      // kind = base kind (0 range, 1 not-range, 2 code set, 3 col-col range) | OR-group << 8 (0: top level)
      const int base = kind & 0xff, grp = kind >> 8;
      if (col < 0 || col >= f.ncols || kind < 0 || base > 3 || grp > 31 || (base == 3 && (int64_t)set >= f.ncols))
        throw std::runtime_error("fused scan: bad term");
      f.terms[i] = kern::FfTerm{col, kind, lo, hi, set};
    }
    f.mask = P<const uint8_t>(mask);
    return f;
  };
  m.def("ff_mask", [make_ff](const FfCols& cols, const FfTerms& terms, uintptr_t mask, int64_t n, uintptr_t out,
                             uintptr_t s) {
    kern::FfSpec f = make_ff(cols, terms, mask);
    kern::ff_mask(f, n, P<uint8_t>(out), S(s));
  });
  m.def("ff_aggregate", [make_ff](const FfCols& cols, const FfTerms& terms, uintptr_t mask, const FfKeys& keys,
                                  int ngroups, const FfAggs& aggs, uintptr_t counts, uintptr_t overflow, int64_t n,
                                  uintptr_t s) {
    kern::FfSpec f = make_ff(cols, terms, mask);
    if (keys.size() > 2 || ngroups < 1 || ngroups > kern::kFfMaxGroups || aggs.size() > (size_t)kern::kFfMaxAggs)
      throw std::runtime_error("fused aggregate: shape out of range");
    f.nkeys = (int32_t)keys.size();
    for (size_t i = 0; i < keys.size(); ++i) {
      auto [col, lo, mul] = keys[i];
      if (col < 0 || col >= f.ncols) throw std::runtime_error("fused aggregate: bad key column");
      f.key_col[i] = col;
      f.key_lo[i] = lo;
      f.key_mul[i] = mul;
    }
    f.ngroups = ngroups;
    f.naggs = (int32_t)aggs.size();
    for (size_t i = 0; i < aggs.size(); ++i) {
      auto& [op, checked, facs, dst, dst2, shared, vbits] = aggs[i];
      if (op < 0 || op > 3 || facs.size() > (size_t)kern::kFfMaxFactors)
        throw std::runtime_error("fused aggregate: bad aggregate");
      if (shared < 0 || shared > (int)facs.size() || (shared > 0 && (i == 0 || f.aggs[i - 1].nfac != shared)))
        throw std::runtime_error("fused aggregate: bad shared prefix");
      kern::FfAgg& A = f.aggs[i];
      A.op = op;
      A.checked = checked;
      A.shared = shared;
      A.nfac = (int32_t)facs.size();
      for (size_t k = 0; k < facs.size(); ++k) {
        auto [col, a, b] = facs[k];
        if (col >= f.ncols) throw std::runtime_error("fused aggregate: bad factor column");
        A.f[k] = kern::FfFactor{col, a, b};
      }
      A.dst = P<int64_t>(dst);
      A.dst2 = P<int64_t>(dst2);
      A.vbits = vbits > 0 && vbits < 64 ? vbits : 64;
    }
    f.counts = P<int64_t>(counts);
    f.overflow = P<int>(overflow);
    kern::ff_aggregate(f, n, S(s));
  });
  m.def("ff_set_mfma", &kern::ff_set_mfma);
  m.attr("HLL_REGISTERS") = kern::kHllRegisters;
  m.def("hll_blocks", &kern::hll_blocks);
  m.def("hll_sketch", raw<&kern::hll_sketch>);
  m.def("groupby_build", raw<&kern::groupby_build>);
  m.def("groupby_occupied", raw<&kern::groupby_occupied>);
  m.def("groupby_assign", raw<&kern::groupby_assign>);
  m.def("groupby_lookup", raw<&kern::groupby_lookup>);
  m.def("fill_runs", raw<&kern::fill_runs>);

  // ------------------------------------------------------------ aggregation
  m.def("agg_lds_max_groups", &kern::agg_lds_max_groups);
  // descs: list of (op, src64, src, valid, dst, dst2)
  m.def("agg_update", [](uintptr_t gid, int64_t n, int ngroups, const AggDescArg& descs, uintptr_t s,
                         bool sorted_gids) {
    auto d = agg_descs(descs);
    kern::agg_update(P<const int32_t>(gid), n, ngroups, d.data(), (int)d.size(), S(s), sorted_gids);
  }, py::arg("gid"), py::arg("n"), py::arg("ngroups"), py::arg("descs"), py::arg("s"), py::arg("sorted_gids") = false);
  // ---- moments.hip
  m.def("agg_moments2", raw<&kern::agg_moments2>);
  m.attr("MOMENTS_LDS_MAX_GROUPS") = (int)kern::kMomentsLdsMaxGroups;
  m.attr("MOMENTS_ROWS_PER_BLOCK") = (int)kern::kMomentsRowsPerBlock;
  m.def("agg_part_buckets", &kern::agg_part_buckets);
  m.def("agg_part_blocks", &kern::agg_part_blocks);
  // phase 0 / 1 / 2 of the radix-partitioned aggregate; vals: one pointer per desc (0: COUNT(*))
  m.def("agg_partitioned", [](uintptr_t gid, int64_t n, int64_t ngroups, const AggDescArg& descs, int phase,
                              uintptr_t cnt, uintptr_t off, uintptr_t total, uintptr_t pg,
                              const std::vector<uintptr_t>& vals, uintptr_t s) {
    if (!gid || n >= (int64_t(1) << 31) || ngroups <= 0 || ngroups >= (int64_t(1) << 31) || phase < 0 || phase > 2 ||
        descs.empty() || descs.size() > 8 || vals.size() != descs.size() || (phase == 0 && !cnt) ||
        (phase >= 1 && (!off || !pg)) || (phase == 2 && !total))
      throw std::runtime_error("agg_partitioned: bad arguments");
    auto d = agg_descs(descs);
    std::vector<int64_t*> v;
    for (auto x : vals) v.push_back(P<int64_t>(x));
    kern::agg_partitioned(P<const int32_t>(gid), n, ngroups, d.data(), (int)d.size(), phase, P<int32_t>(cnt),
                          P<const int64_t>(off), P<const int64_t>(total), P<uint16_t>(pg), v.data(), S(s));
  });
  m.def("sorted_having", [](uintptr_t keys, bool key64, int64_t n, const AggDescArg& descs, int hagg, int hop,
                            long long hlo, long long hhi, double hf, uintptr_t rep, int64_t cap, uintptr_t counter,
                            uintptr_t s) {
    auto d = agg_descs(descs);
    kern::sorted_having(P<const void>(keys), key64, n, d.data(), (int)d.size(), hagg, hop, hlo, hhi, hf,
                        P<int64_t>(rep), cap, P<unsigned long long>(counter), S(s));
  });
  m.def("key_histogram", [](uintptr_t keys, bool key64, uintptr_t valid, int64_t n, int64_t kmin, int64_t span,
                            uintptr_t counts, uintptr_t s) {
    if (n > 0 && (!keys || !counts || span <= 0)) throw std::runtime_error("key_histogram: bad arguments");
    kern::key_histogram(P<const void>(keys), key64, P<const uint8_t>(valid), n, kmin, span, P<int32_t>(counts), S(s));
  });
  m.def("key_histogram_buckets", &kern::key_histogram_buckets);
  m.def("key_histogram_blocks", &kern::key_histogram_blocks);
  m.def("key_histogram_partitioned", [](uintptr_t keys, bool key64, uintptr_t valid, int64_t n, int64_t kmin,
                                        int64_t span, int phase, uintptr_t cnt, uintptr_t off, int64_t total,
                                        uintptr_t part, uintptr_t counts, uintptr_t s) {
    if (span <= 0 || span > (int64_t(1) << 27) || n >= (int64_t(1) << 31) || phase < 0 || phase > 2 || !keys ||
        (phase == 0 && !cnt) || (phase >= 1 && (!off || !part)) || (phase == 2 && !counts))
      throw std::runtime_error("key_histogram_partitioned: bad arguments");
    kern::key_histogram_partitioned(P<const void>(keys), key64, P<const uint8_t>(valid), n, kmin, span, phase,
                                    P<int32_t>(cnt), P<const int64_t>(off), total, P<uint16_t>(part),
                                    P<int32_t>(counts), S(s));
  });

  // ----------------------------------------------------------------- gather
  // descs: list of (src, dst, elem_bytes, src_valid, dst_valid, src_rows)
  m.def("gather_multi", [](uintptr_t idx, bool idx64, int64_t n, const std::vector<std::tuple<uintptr_t, uintptr_t, int, uintptr_t, uintptr_t, int64_t>>& descs, uintptr_t s) {
    std::vector<kern::GatherDesc> d;
    for (auto& t : descs)
      d.push_back({P<const void>(std::get<0>(t)), P<void>(std::get<1>(t)), std::get<2>(t),
                   P<const uint8_t>(std::get<3>(t)), P<uint8_t>(std::get<4>(t)), std::get<5>(t)});
    kern::gather_multi(P<const void>(idx), idx64, n, d.data(), (int)d.size(), S(s));
  });
  m.def("gather_packed", [](uintptr_t idx, bool idx64, int64_t n, uintptr_t src, int64_t rows, int row_bytes,
                            const std::vector<std::tuple<uintptr_t, int, int, int, int>>& fields, uintptr_t s) {
    std::vector<kern::PackedField> f;
    for (auto& t : fields)
      f.push_back({P<void>(std::get<0>(t)), std::get<1>(t), std::get<2>(t), std::get<3>(t), std::get<4>(t)});
    kern::gather_packed(P<const void>(idx), idx64, n, P<const uint8_t>(src), rows, row_bytes, f.data(), (int)f.size(),
                        S(s));
  });
  m.def("str_gather_lengths", raw<&kern::str_gather_lengths>);
  m.def("str_gather_copy", raw<&kern::str_gather_copy>);

  // ---------------------------------------------------------------- strings
  m.def("str_like", raw<&kern::str_like>);
  m.def("str_case", raw<&kern::str_case>);
  m.def("str_substr_lengths", raw<&kern::str_substr_lengths>);
  m.def("str_substr_copy", raw<&kern::str_substr_copy>);
  m.def("str_char_length", raw<&kern::str_char_length>);
  m.def("str_concat2_lengths", raw<&kern::str_concat2_lengths>);
  m.def("str_concat2_copy", raw<&kern::str_concat2_copy>);
  m.def("fmt_lengths", raw<&kern::fmt_lengths>);
  m.def("fmt_write", raw<&kern::fmt_write>);
  m.def("str_parse", raw<&kern::str_parse>);
  m.def("try_parse", raw<&kern::try_parse>);
  m.def("cast_checked", raw<&kern::cast_checked>);
  m.def("str_prefix_keys", raw<&kern::str_prefix_keys>);
  m.def("str_hash64", raw<&kern::str_hash64>);
  m.def("str_like_segments", raw<&kern::str_like_segments>);
  m.def("str_eq_rows", raw<&kern::str_eq_rows>);
  m.def("str_in_set", [](uintptr_t off, uintptr_t chars, int64_t n, uintptr_t vb, uintptr_t voff, uintptr_t vmode,
                         int nv, uintptr_t out, uintptr_t s) {
    if (n > 0 && (!off || !out || nv < 0 || (nv > 0 && (!vb || !voff || !vmode))))
      throw std::runtime_error("str_in_set: bad arguments");
    kern::str_in_set(P<const int64_t>(off), P<const uint8_t>(chars), n, P<const uint8_t>(vb), P<const int32_t>(voff),
                     P<const uint8_t>(vmode), nv, P<uint8_t>(out), S(s));
  });
  m.def("str_cmp_const", raw<&kern::str_cmp_const>);
  m.def("str_prefix_key", raw<&kern::str_prefix_key>);

  // -------------------------------------------------------------------- csv
  m.attr("CSV_TILE") = kern::kCsvTile;
  m.attr("CSV_COLUMN_BYTES") = (int)sizeof(kern::CsvColumn);
  m.def("csv_num_tiles", &kern::csv_num_tiles);
  m.def("csv_quote_parity", [](uintptr_t buf, int64_t n, int quote, uintptr_t tile_par, uintptr_t s) {
    kern::csv_quote_parity(P<const uint8_t>(buf), n, (uint8_t)quote, P<uint8_t>(tile_par), S(s));
  });
  m.def("csv_rows", [](uintptr_t buf, int64_t n, int64_t start, int quote, uintptr_t tile_state, uintptr_t tile_rows,
                       uintptr_t tile_off, uintptr_t rows_end, uintptr_t s) {
    kern::csv_rows(P<const uint8_t>(buf), n, start, (uint8_t)quote, P<const uint8_t>(tile_state),
                   P<int64_t>(tile_rows), P<const int64_t>(tile_off), P<int64_t>(rows_end), S(s));
  });
  // cols: [(kind, scale, out, len, valid)] -> packed CsvColumn array (upload, then pass to csv_parse)
  m.def("csv_pack_columns", [](const std::vector<std::tuple<int, int, uintptr_t, uintptr_t, uintptr_t>>& cols) {
    std::vector<kern::CsvColumn> v;
    for (auto& [kind, scale, out, len, valid] : cols) {
      if (kind < kern::CSV_SKIP || kind > kern::CSV_UTF8) throw std::runtime_error("csv: bad column kind");
      if (kind != kern::CSV_SKIP && !out) throw std::runtime_error("csv: missing output buffer");
      if (kind == kern::CSV_UTF8 && !len) throw std::runtime_error("csv: missing length buffer");
      v.push_back({kind, scale, P<void>(out), P<int64_t>(len), P<uint8_t>(valid)});
    }
    return py::bytes(reinterpret_cast<const char*>(v.data()), v.size() * sizeof(kern::CsvColumn));
  });
  m.def("csv_parse", [](uintptr_t buf, int64_t start, uintptr_t rows_end, int64_t nrows, uintptr_t cols, int ncols,
                        int delim, int quote, uintptr_t err, uintptr_t s) {
    kern::csv_parse(P<const uint8_t>(buf), start, P<const int64_t>(rows_end), nrows,
                    P<const kern::CsvColumn>(cols), ncols, (uint8_t)delim, (uint8_t)quote, P<int>(err), S(s));
  });
  m.def("csv_str_lengths", raw<&kern::csv_str_lengths>);
  m.def("csv_str_copy", [](uintptr_t pos, uintptr_t len_flag, uintptr_t off, int64_t n, int quote, uintptr_t out,
                           uintptr_t s) {
    kern::csv_str_copy(P<const int64_t>(pos), P<const int64_t>(len_flag), P<const int64_t>(off), n, (uint8_t)quote,
                       P<uint8_t>(out), S(s));
  });

  m.def("strfmt_lengths", [](const std::string& fmt, bool is_date, uintptr_t v, uintptr_t offs, int64_t n,
                             uintptr_t len, uintptr_t s) {
    kern::strfmt_lengths(reinterpret_cast<const uint8_t*>(fmt.data()), (int)fmt.size(), is_date, P<const void>(v),
                         P<const int32_t>(offs), n, P<int64_t>(len), S(s));
  });
  m.def("strfmt_write", [](const std::string& fmt, bool is_date, uintptr_t v, uintptr_t offs, int64_t n,
                           uintptr_t off, int64_t out_cap, uintptr_t out, uintptr_t s) {
    kern::strfmt_write(reinterpret_cast<const uint8_t*>(fmt.data()), (int)fmt.size(), is_date, P<const void>(v),
                       P<const int32_t>(offs), n, P<const int64_t>(off), out_cap, P<uint8_t>(out), S(s));
  });
  m.def("strptime", raw<&kern::strptime>);
  m.def("tz_to_local", raw<&kern::tz_to_local>);
  m.def("tz_to_utc", raw<&kern::tz_to_utc>);
  m.def("tz_trunc", raw<&kern::tz_trunc>);
  m.def("tz_part", raw<&kern::tz_part>);
  m.def("regex_lds_bytes", &kern::regex_lds_bytes);
  m.def("regex_dfa_match", raw<&kern::regex_dfa_match>);
  // span automaton as (table, cls, flags, nstates, nclasses, anchored_start, anchored_end)
  using SpanDfaArg = std::tuple<uintptr_t, uintptr_t, uintptr_t, int, int, bool, bool>;
  auto span_dfa = [](const SpanDfaArg& d) {
    return kern::RegexSpanDfa{P<const uint16_t>(std::get<0>(d)), P<const uint8_t>(std::get<1>(d)),
                              P<const uint8_t>(std::get<2>(d)), std::get<3>(d), std::get<4>(d), std::get<5>(d),
                              std::get<6>(d)};
  };
  m.def("regex_span_count", [span_dfa](const SpanDfaArg& d, uintptr_t off, uintptr_t chars, int64_t n, bool all,
                                       int64_t repl_len, int64_t start_char, uintptr_t out, uintptr_t exhausted,
                                       uintptr_t s) {
    kern::regex_span_count(span_dfa(d), P<const int64_t>(off), P<const uint8_t>(chars), n, all, repl_len, start_char,
                           P<int64_t>(out), P<int64_t>(exhausted), S(s));
  });
  m.def("regex_span_first", [span_dfa](const SpanDfaArg& d, uintptr_t off, uintptr_t chars, int64_t n,
                                       uintptr_t out_pos, uintptr_t out_len, uintptr_t exhausted, uintptr_t s) {
    kern::regex_span_first(span_dfa(d), P<const int64_t>(off), P<const uint8_t>(chars), n, P<int64_t>(out_pos),
                           P<int64_t>(out_len), P<int64_t>(exhausted), S(s));
  });
  m.def("regex_span_replace", [span_dfa](const SpanDfaArg& d, uintptr_t off, uintptr_t chars, int64_t n, bool all,
                                         uintptr_t repl, int64_t repl_len, uintptr_t new_off, uintptr_t out,
                                         int64_t cap, uintptr_t s) {
    kern::regex_span_replace(span_dfa(d), P<const int64_t>(off), P<const uint8_t>(chars), n, all,
                             P<const uint8_t>(repl), repl_len, P<const int64_t>(new_off), P<uint8_t>(out), cap, S(s));
  });
  m.def("probe_hash16", raw<&kern::probe_hash16>);
  m.def("probe_inlist16", [](bool mfma, uintptr_t off, uintptr_t chars, int64_t n, const std::string& pats, int npat,
                             int len, uintptr_t out, uintptr_t s) {
    if ((int64_t)pats.size() < 16 * npat) throw std::runtime_error("probe_inlist16: 16 bytes per pattern");
    kern::probe_inlist16(mfma, P<const int64_t>(off), P<const uint8_t>(chars), n,
                         reinterpret_cast<const uint8_t*>(pats.data()), npat, len, P<uint8_t>(out), S(s));
  });
  m.def("digest_width", &kern::digest_width);
  m.def("digest_hex", raw<&kern::digest_hex>);
  m.def("bin_hex_encode", raw<&kern::bin_hex_encode>);
  m.def("bin_hex_validate", raw<&kern::bin_hex_validate>);
  m.def("bin_hex_decode", raw<&kern::bin_hex_decode>);
  m.def("bin_b64_enc_lengths", raw<&kern::bin_b64_enc_lengths>);
  m.def("bin_b64_dec_lengths", raw<&kern::bin_b64_dec_lengths>);
  m.def("bin_b64_write", raw<&kern::bin_b64_write>);
  m.def("utf8_num_tiles", &kern::utf8_num_tiles);
  m.def("utf8_validate", raw<&kern::utf8_validate>);
  m.def("uuid_v4", raw<&kern::uuid_v4>);
  m.def("list_element_idx", raw<&kern::list_element_idx>);
  m.def("interleave_idx", raw<&kern::interleave_idx>);
  m.def("list_slots", raw<&kern::list_slots>);
  m.attr("LIST_FAST_MAX") = (int)kern::kListFastMax;
  m.def("map_lookup_idx", raw<&kern::map_lookup_idx>);
  m.def("map_lookup_idx_str", raw<&kern::map_lookup_idx_str>);
  m.def("list_slice_se", raw<&kern::list_slice_se>);
  m.def("list_parts_count", raw<&kern::list_parts_count>);
  m.def("list_parts_write", raw<&kern::list_parts_write>);
  m.def("list_flatten_count", raw<&kern::list_flatten_count>);
  m.def("list_flatten_write", raw<&kern::list_flatten_write>);
  m.def("list_match_count", raw<&kern::list_match_count>);
  m.def("list_match_write", raw<&kern::list_match_write>);
  m.def("list_minmax_idx", raw<&kern::list_minmax_idx>);
  m.def("list_set_count", raw<&kern::list_set_count>);
  m.def("list_set_write", raw<&kern::list_set_write>);
  m.def("list_sort_idx", raw<&kern::list_sort_idx>);
  m.def("json_parse", [](uintptr_t buf, int64_t start, uintptr_t rows_end, int64_t nrows, uintptr_t cols, int ncols,
                         uintptr_t names, uintptr_t name_off, uintptr_t err, uintptr_t s) {
    if (ncols > 64) throw std::runtime_error("json_parse: at most 64 fields");
    kern::json_parse(P<const uint8_t>(buf), start, P<const int64_t>(rows_end), nrows, P<const kern::CsvColumn>(cols),
                     ncols, P<const uint8_t>(names), P<const int32_t>(name_off), P<int>(err), S(s));
  });
  m.def("json_str_copy", raw<&kern::json_str_copy>);

  // ----------------------------------------------------------- sorted joins
  m.def("sorted_ranges", raw<&kern::sorted_ranges>);
  m.attr("SEARCH_FENCE") = kern::kFence;
  m.attr("STATS_SLOTS") = kern::kStatsSlots;
  m.def("expand_ranges", raw<&kern::expand_ranges>);

  m.def("dense_index_build", [](uintptr_t big, bool key64, int64_t nb, int64_t kmin, int64_t kmax, uintptr_t first,
                                bool first64, uintptr_t long_gap, uintptr_t s) {
    if (nb <= 0 || kmax < kmin || !big || !first) throw std::runtime_error("dense_index_build: bad arguments");
    kern::dense_index_build(P<const void>(big), key64, nb, kmin, kmax, P<void>(first), first64, P<int32_t>(long_gap),
                            S(s));
  });
  m.def("dense_ranges", [](uintptr_t first, bool first64, int64_t kmin, int64_t kmax, uintptr_t q, bool key64,
                           uintptr_t qvalid, int64_t nq, uintptr_t lo, uintptr_t cnt, uintptr_t s) {
    if (nq > 0 && (!first || !q || !lo || !cnt)) throw std::runtime_error("dense_ranges: null buffer");
    kern::dense_ranges(P<const void>(first), first64, kmin, kmax, P<const void>(q), key64, P<const uint8_t>(qvalid), nq,
                       P<int64_t>(lo), P<int64_t>(cnt), S(s));
  });
  m.def("unique_lookup", [](uintptr_t big, bool key64, int64_t nb, uintptr_t first, bool first64, int64_t kmin,
                            int64_t kmax, uintptr_t q, uintptr_t qvalid, int64_t nq, uintptr_t hit, uintptr_t pos,
                            uintptr_t fence, int64_t nf, uintptr_t s) {
    if (nq > 0 && (!q || !hit || !pos || (!first && !big))) throw std::runtime_error("unique_lookup: null buffer");
    if (nb >= (int64_t{1} << 31)) throw std::runtime_error("unique_lookup: positions must fit int32");
    kern::unique_lookup(P<const void>(big), key64, nb, P<const void>(first), first64, kmin, kmax, P<const void>(q),
                        P<const uint8_t>(qvalid), nq, P<uint8_t>(hit), P<int32_t>(pos), P<const void>(fence), nf,
                        S(s));
  });
  // two-level rank index (ranges.hip): build steps, then the lookups through it
  m.def("rank_index_bits", [](uintptr_t big, bool key64, int64_t nb, int64_t kmin, int64_t kmax, uintptr_t entries,
                              uintptr_t s) {
    if (nb <= 0 || kmax < kmin || !big || !entries || (entries & 15))
      throw std::runtime_error("rank_index_bits: bad arguments");
    kern::rank_index_bits(P<const void>(big), key64, nb, kmin, kmax, P<void>(entries), S(s));
  });
  m.def("rank_index_counts", [](uintptr_t entries, int64_t nwords, uintptr_t counts, uintptr_t s) {
    if (nwords <= 0 || !entries || !counts) throw std::runtime_error("rank_index_counts: bad arguments");
    kern::rank_index_counts(P<const void>(entries), nwords, P<int32_t>(counts), S(s));
  });
  m.def("rank_index_finish", [](uintptr_t entries, int64_t nwords, uintptr_t offsets, uintptr_t s) {
    if (nwords <= 0 || !entries || !offsets) throw std::runtime_error("rank_index_finish: bad arguments");
    kern::rank_index_finish(P<void>(entries), nwords, P<const int64_t>(offsets), S(s));
  });
  m.def("rank_index_starts", [](uintptr_t big, bool key64, int64_t nb, int64_t kmin, int64_t kmax, uintptr_t entries,
                                uintptr_t starts, bool starts64, int64_t nd, uintptr_t s) {
    if (nb <= 0 || kmax < kmin || nd < 0 || !big || !entries || !starts)
      throw std::runtime_error("rank_index_starts: bad arguments");
    kern::rank_index_starts(P<const void>(big), key64, nb, kmin, kmax, P<const void>(entries), P<void>(starts),
                            starts64, nd, S(s));
  });
  m.def("rank_ranges", [](uintptr_t entries, uintptr_t starts, bool starts64, int64_t nd, int64_t kmin, int64_t kmax,
                          uintptr_t q, bool key64, uintptr_t qvalid, int64_t nq, uintptr_t lo, uintptr_t cnt,
                          uintptr_t s) {
    if (kmax < kmin || (entries & 15) || (nq > 0 && (!q || !lo || !cnt)))
      throw std::runtime_error("rank_ranges: bad arguments");
    kern::rank_ranges(P<const void>(entries), P<const void>(starts), starts64, nd, kmin, kmax, P<const void>(q), key64,
                      P<const uint8_t>(qvalid), nq, P<int64_t>(lo), P<int64_t>(cnt), S(s));
  });
  m.def("rank_unique", [](uintptr_t entries, uintptr_t starts, bool starts64, int64_t nd, int64_t kmin, int64_t kmax,
                          uintptr_t q, bool key64, uintptr_t qvalid, int64_t nq, uintptr_t hit, uintptr_t pos,
                          uintptr_t s) {
    if (kmax < kmin || (entries & 15) || (nq > 0 && (!q || !hit || !pos)))
      throw std::runtime_error("rank_unique: bad arguments");
    kern::rank_unique(P<const void>(entries), P<const void>(starts), starts64, nd, kmin, kmax, P<const void>(q), key64,
                      P<const uint8_t>(qvalid), nq, P<uint8_t>(hit), P<int32_t>(pos), S(s));
  });
  m.def("sorted_exists", [](uintptr_t big2, uintptr_t small2, bool key64, uintptr_t lo, uintptr_t cnt, int64_t ns,
                            int op, uintptr_t mask, uintptr_t hit, uintptr_t s) {
    // op 6 (any row of the range set in mask) reads neither value column
    if (op < 0 || op > 6 || (op == 6 && !mask) || (ns > 0 && (!lo || !cnt || !hit || (op < 6 && (!big2 || !small2)))))
      throw std::runtime_error("sorted_exists: bad arguments");
    kern::sorted_exists(P<const void>(big2), P<const void>(small2), key64, P<const int64_t>(lo), P<const int64_t>(cnt),
                        ns, op, P<const uint8_t>(mask), P<uint8_t>(hit), S(s));
  });
  m.def("sorted_match", [](uintptr_t big2, uintptr_t small2, bool key64, uintptr_t lo, uintptr_t cnt, int64_t ns,
                           uintptr_t counts, uintptr_t offsets, uintptr_t sidx, uintptr_t bidx, bool out64,
                           int64_t out_cap, uintptr_t first, uintptr_t s) {
    if (ns > 0 && (!big2 || !small2 || !lo || !cnt || (!offsets && !counts) || (offsets && (!sidx || !bidx))))
      throw std::runtime_error("sorted_match: null buffer");
    kern::sorted_match(P<const void>(big2), P<const void>(small2), key64, P<const int64_t>(lo), P<const int64_t>(cnt),
                       ns, P<int32_t>(counts), P<const int64_t>(offsets), P<void>(sidx), P<void>(bidx), out64,
                       out_cap, P<int32_t>(first), S(s));
  });
  m.def("sorted_masked", [](uintptr_t mask, uintptr_t lo, uintptr_t cnt, int64_t ns, uintptr_t counts,
                            uintptr_t offsets, uintptr_t sidx, uintptr_t bidx, bool out64, int64_t out_cap,
                            uintptr_t s) {
    if (ns > 0 && (!mask || !lo || !cnt || (!offsets && !counts) || (offsets && (!sidx || !bidx))))
      throw std::runtime_error("sorted_masked: null buffer");
    kern::sorted_masked(P<const uint8_t>(mask), P<const int64_t>(lo), P<const int64_t>(cnt), ns, P<int32_t>(counts),
                        P<const int64_t>(offsets), P<void>(sidx), P<void>(bidx), out64, out_cap, S(s));
  });

  // -------------------------------------------------------------- partition
  m.def("partition_run_blocks", &kern::partition_run_blocks);
  m.def("partition_run", raw<&kern::partition_run>);
  m.def("partition_ids", raw<&kern::partition_ids>);
  m.def("date_part", raw<&kern::date_part>);
  m.def("str_fn_lengths", [](int fn, int64_t n1, uintptr_t a, int64_t alen, uintptr_t b, int64_t blen, uintptr_t off,
                             uintptr_t chars, int64_t n, uintptr_t len, uintptr_t s) {
    kern::StrFnArgs args{fn, n1, P<uint8_t>(a), alen, P<uint8_t>(b), blen};
    kern::str_fn_lengths(args, P<int64_t>(off), P<uint8_t>(chars), n, P<int64_t>(len), S(s));
  });
  m.def("str_fn_copy", [](int fn, int64_t n1, uintptr_t a, int64_t alen, uintptr_t b, int64_t blen, uintptr_t off,
                          uintptr_t chars, int64_t n, uintptr_t new_off, uintptr_t out, int64_t out_cap,
                          uintptr_t s) {
    kern::StrFnArgs args{fn, n1, P<uint8_t>(a), alen, P<uint8_t>(b), blen};
    kern::str_fn_copy(args, P<int64_t>(off), P<uint8_t>(chars), n, P<int64_t>(new_off), P<uint8_t>(out), out_cap,
                      S(s));
  });
  m.def("str_fn_int", raw<&kern::str_fn_int>);
  m.attr("LEV_FAST_MAX") = (int)kern::kLevFastMax;
  m.def("str_pair_int", raw<&kern::str_pair_int>);
  m.def("str_levenshtein", raw<&kern::str_levenshtein>);
  m.def("str_levenshtein_long", raw<&kern::str_levenshtein_long>);
  m.def("str_row_cmp", raw<&kern::str_row_cmp>);
  m.def("win_scan_tiles", &kern::win_scan_tiles);
  m.def("win_seg_scan", raw<&kern::win_seg_scan>);
  m.def("win_bounds", raw<&kern::win_bounds>);
  m.def("win_frame_sum", raw<&kern::win_frame_sum>);
  m.def("win_sparse_build", raw<&kern::win_sparse_build>);
  m.def("win_sparse_query", raw<&kern::win_sparse_query>);
  m.def("win_frame_minmax", raw<&kern::win_frame_minmax>);
  m.def("win_rank", raw<&kern::win_rank>);
  m.def("win_index", raw<&kern::win_index>);
  m.def("win_frame_kth", raw<&kern::win_frame_kth>);
  m.def("win_select_tile", &kern::win_select_tile);
  m.def("win_select_levels", &kern::win_select_levels);
  m.def("win_select_build", raw<&kern::win_select_build>);
  m.def("win_select_query", raw<&kern::win_select_query>);

  // ---------------------------------------------------------------- parquet
  m.def("pq_file_meta", [](const std::string& path) {
    io::PqFileMeta meta;
    {
      py::gil_scoped_release rel;
      meta = io::read_file_meta(path);
    }
    py::dict d;
    d["version"] = meta.version;
    d["num_rows"] = meta.num_rows;
    d["created_by"] = meta.created_by;
    py::list leaves, groups;
    for (auto& l : meta.leaves) leaves.append(leaf_dict(l));
    for (auto& g : meta.row_groups) {
      py::dict gd;
      gd["num_rows"] = g.num_rows;
      py::list cs;
      for (auto& c : g.chunks) cs.append(chunk_dict(c));
      gd["chunks"] = cs;
      groups.append(gd);
    }
    d["leaves"] = leaves;
    d["row_groups"] = groups;
    return d;
  }, "Parse a Parquet footer (native Thrift compact decoder)");
  m.def("pq_page_headers", [](uintptr_t host, int64_t n) {
    py::list out;
    for (auto& h : io::parse_chunk_pages(P<const uint8_t>(host), (size_t)n)) out.append(page_header_dict(h));
    return out;
  });
  m.def("pq_pread", [](const std::string& path, const std::vector<std::tuple<int64_t, int64_t, uintptr_t>>& ranges,
                       int threads) {
    std::vector<io::ReadRange> rs;
    for (auto& [off, len, dst] : ranges) {
      if (off < 0 || len < 0 || !dst) throw std::runtime_error("pq_pread: bad range");
      rs.push_back({off, len, P<uint8_t>(dst)});
    }
    py::gil_scoped_release rel;
    io::pread_ranges(path, rs, threads);
  });
  // chunks: (buffer offset, bytes, codec, first row, rows[, values]) — `values` (the footer's
  // num_values) bounds the page walk of a repeated leaf, whose pages count entries
  m.def("pq_plan", [](uintptr_t host, const std::vector<py::tuple>& chunks, int phys, int max_def, int max_rep,
                      int64_t dec_base, int type_len, bool levels) {
    std::vector<io::PqChunkIn> cs;
    for (auto& c : chunks) {
      if (c.size() != 5 && c.size() != 6) throw std::runtime_error("pq_plan: a chunk is 5 or 6 numbers");
      cs.push_back({c[0].cast<int64_t>(), c[1].cast<int64_t>(), c[2].cast<int>(), c[3].cast<int64_t>(),
                    c[4].cast<int64_t>(), c.size() == 6 ? c[5].cast<int64_t>() : -1});
    }
    io::PqPlan plan;
    {
      py::gil_scoped_release rel;
      plan = io::plan_column(P<const uint8_t>(host), cs, phys, max_def, max_rep, dec_base, type_len, levels);
    }
    py::dict d;
    d["pages"] = py::bytes((const char*)plan.pages.data(), plan.pages.size());
    d["jobs"] = py::bytes((const char*)plan.jobs.data(), plan.jobs.size());
    d["level_pages"] = py::bytes((const char*)plan.level_pages.data(), plan.level_pages.size());
    d["num_level_pages"] = plan.num_level_pages;
    d["num_entries"] = plan.num_entries;
    d["num_pages"] = plan.num_pages;
    d["num_jobs"] = plan.num_jobs;
    d["num_zstd_jobs"] = plan.num_zstd_jobs;
    d["num_dict_pages"] = plan.num_dict_pages;
    d["dec_bytes"] = plan.dec_bytes;
    d["dict_entries"] = plan.dict_entries;
    d["plain_pages"] = plan.plain_pages;
    d["max_page_values"] = plan.max_page_values;
    d["unsupported"] = plan.unsupported;
    return d;
  }, "Plan GPU decode descriptors for one column's chunks staged at `host`",
     py::arg("host"), py::arg("chunks"), py::arg("phys"), py::arg("max_def"), py::arg("max_rep"),
     py::arg("dec_base") = 0, py::arg("type_len") = 0, py::arg("levels") = false);
  m.def("pq_pack_spec", [](const py::dict& spec, bool need_output) {
    kern::PqDecodeSpec sp = decode_spec(spec, need_output);
    return py::bytes(reinterpret_cast<const char*>(&sp), sizeof(sp));
  }, "Validated binary PqDecodeSpec (concatenate one per column and upload)");
  m.attr("PQ_SPEC_BYTES") = (int)sizeof(kern::PqDecodeSpec);
  m.attr("PQ_LEVEL_PAGE_BYTES") = (int)sizeof(kern::PqLevelPage);
  m.def("pq_zstd_slots", &kern::pq_zstd_slots);
  m.def("pq_zstd", [](uintptr_t jobs, int64_t njobs, uintptr_t raw, uintptr_t dec, uintptr_t lit, int64_t slots,
                      uintptr_t err, uintptr_t s) {
    if (njobs > 0 && (!jobs || !raw || !dec || !lit || !err)) throw std::runtime_error("pq_zstd: null buffer");
    kern::pq_zstd(P<const kern::PqSnappyJob>(jobs), njobs, P<const uint8_t>(raw), P<uint8_t>(dec), P<uint8_t>(lit),
                  slots, P<int>(err), S(s));
  });
  // host reference: decompress `src` (bytes) into exactly `size` bytes; (error code, output)
  m.def("zstd_decompress_host", [](py::bytes src, int64_t size) {
    std::string in = src;
    std::string out((size_t)size, '\0');
    int e;
    {
      py::gil_scoped_release nogil;
      e = kern::zstd_decompress_host((const uint8_t*)in.data(), (int64_t)in.size(), (uint8_t*)out.data(), size);
    }
    return py::make_tuple(e, py::bytes(out));
  });
  m.def("pq_snappy", [](uintptr_t jobs, int64_t njobs, uintptr_t raw, uintptr_t dec, uintptr_t err, uintptr_t s) {
    if (njobs > 0 && (!jobs || !raw || !dec || !err)) throw std::runtime_error("pq_snappy: null buffer");
    kern::pq_snappy(P<const kern::PqSnappyJob>(jobs), njobs, P<const uint8_t>(raw), P<uint8_t>(dec), P<int>(err), S(s));
  });
  m.def("pq_dict_strings", [](uintptr_t pages, int64_t npages, uintptr_t page_col, uintptr_t specs, uintptr_t s) {
    if (npages > 0 && (!pages || !page_col || !specs)) throw std::runtime_error("pq_dict_strings: null buffer");
    kern::pq_dict_strings(P<const kern::PqPage>(pages), npages, P<const int32_t>(page_col),
                          P<const kern::PqDecodeSpec>(specs), S(s));
  });
  m.def("pq_decode", [](uintptr_t pages, int64_t npages, uintptr_t page_col, uintptr_t specs, uintptr_t s) {
    if (npages > 0 && (!pages || !page_col || !specs)) throw std::runtime_error("pq_decode: null buffer");
    kern::pq_decode(P<const kern::PqPage>(pages), npages, P<const int32_t>(page_col),
                    P<const kern::PqDecodeSpec>(specs), S(s));
  });
  m.def("pq_str_copy", raw<&kern::pq_str_copy>);
  m.def("pq_level_count", raw<&kern::pq_level_count>);
  m.def("pq_list_rows", raw<&kern::pq_list_rows>);
  m.def("pq_list_lens", raw<&kern::pq_list_lens>);
  m.def("pq_struct_valid", raw<&kern::pq_struct_valid>);

  // ---------------------------------------------------------------- datagen
  // params: (kind, seed, row_base, min_len, max_len, vocab, vocab_off, vocab_n,
  //          inject, inject_len, inject_every, suffix_char, aux, row_ids)
  auto mkparams = [](const py::tuple& t) {
    kern::TextGenParams p;
    p.kind = t[0].cast<int>();
    p.seed = t[1].cast<uint64_t>();
    p.row_base = t[2].cast<int64_t>();
    p.min_len = t[3].cast<int>();
    p.max_len = t[4].cast<int>();
    p.vocab = P<const uint8_t>(t[5].cast<uintptr_t>());
    p.vocab_off = P<const int32_t>(t[6].cast<uintptr_t>());
    p.vocab_n = t[7].cast<int>();
    p.inject = P<const uint8_t>(t[8].cast<uintptr_t>());
    p.inject_len = t[9].cast<int>();
    p.inject_every = t[10].cast<int>();
    p.suffix_char = t[11].cast<int>();
    p.aux = P<const int32_t>(t[12].cast<uintptr_t>());
    p.row_ids = t.size() > 13 ? P<const int64_t>(t[13].cast<uintptr_t>()) : nullptr;
    return p;
  };
  m.def("textgen_lengths", [mkparams](const py::tuple& t, int64_t n, uintptr_t lens, bool device, uintptr_t s) {
    auto p = mkparams(t);
    py::gil_scoped_release rel;
    kern::textgen_lengths(p, n, P<int64_t>(lens), device, S(s));
  });
  m.def("textgen_write", [mkparams](const py::tuple& t, int64_t n, uintptr_t off, uintptr_t chars, bool device, uintptr_t s) {
    auto p = mkparams(t);
    py::gil_scoped_release rel;
    kern::textgen_write(p, n, P<const int64_t>(off), P<uint8_t>(chars), device, S(s));
  });
}
