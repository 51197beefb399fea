// Stand-alone sanitizer driver for the TRY_CAST element routines: parse_timestamp of
// csrc/kernels/textparse.h and the checked conversions of csrc/kernels/castcheck.h, compiled as
// plain C++ under ASan / UBSan through the host shim (strpair_host_shim.h as common.h). Every
// text is copied into a heap buffer of its exact size, so a read one byte outside it is an
// AddressSanitizer report; signed overflow or a float -> integer conversion out of range is a
// UBSan report.
//
// stdin, one case per line:
//   T <TAB> 0 <TAB> text                               parse_timestamp -> ok <TAB> microseconds
//   C <TAB> src,src_scale,dst,dst_scale,dst_precision <TAB> value
//        src / dst: the CastKind numbers; value: a decimal integer (up to 128 bits) for integer,
//        decimal and wide sources, the bit pattern in hex for float32 (8 digits) / float64 (16)
//        -> ok <TAB> the converted integer
// A rejected input prints "err". Built and run by tests/test_trycast_host.py (no GPU).
#include "common.h"
#include <cinttypes>
#include <cstdio>
#include <vector>
#include "castcheck.h"
#include "textparse.h"
using namespace igloo::kern;

static __int128 read_i128(const char* s, size_t n) {
  bool neg = n && s[0] == '-';
  unsigned __int128 v = 0;
  for (size_t k = neg; k < n; ++k) v = v * 10 + (unsigned)(s[k] - '0');
  return neg ? (__int128)((unsigned __int128)0 - v) : (__int128)v;
}

template <typename D> static bool to_int(int sk, __int128 iv, uint64_t bits, const CastPlan& p, int64_t* out) {
  D d = 0;
  bool ok;
  switch (sk) {
    case kCastI8: ok = cast_to_int<D>((int8_t)iv, p, &d); break;
    case kCastI16: ok = cast_to_int<D>((int16_t)iv, p, &d); break;
    case kCastI32: ok = cast_to_int<D>((int32_t)iv, p, &d); break;
    case kCastI64: ok = cast_to_int<D>((int64_t)iv, p, &d); break;
    case kCastF32: { float f; uint32_t b = (uint32_t)bits; memcpy(&f, &b, 4); ok = cast_to_int<D>(f, p, &d); break; }
    case kCastF64: { double f; memcpy(&f, &bits, 8); ok = cast_to_int<D>(f, p, &d); break; }
    case kCastDec: ok = cast_to_int<D>(dec_src{(int64_t)iv}, p, &d); break;
    default: ok = cast_to_int<D>(wide_src{(int64_t)(uint64_t)iv, (int64_t)(uint64_t)((unsigned __int128)iv >> 64)}, p, &d);
  }
  *out = (int64_t)d;
  return ok;
}

static bool to_dec(int sk, __int128 iv, uint64_t bits, const CastPlan& p, int64_t* out) {
  switch (sk) {
    case kCastI8: return cast_to_dec((int8_t)iv, p, out);
    case kCastI16: return cast_to_dec((int16_t)iv, p, out);
    case kCastI32: return cast_to_dec((int32_t)iv, p, out);
    case kCastI64: return cast_to_dec((int64_t)iv, p, out);
    case kCastF32: { float f; uint32_t b = (uint32_t)bits; memcpy(&f, &b, 4); return cast_to_dec(f, p, out); }
    case kCastF64: { double f; memcpy(&f, &bits, 8); return cast_to_dec(f, p, out); }
    case kCastDec: return cast_to_dec(dec_src{(int64_t)iv}, p, out);
    default: return cast_to_dec(wide_src{(int64_t)(uint64_t)iv, (int64_t)(uint64_t)((unsigned __int128)iv >> 64)}, p, out);
  }
}

int main() {
  std::vector<char> in;
  char chunk[1 << 16];
  for (size_t n; (n = fread(chunk, 1, sizeof chunk, stdin)) > 0;) in.insert(in.end(), chunk, chunk + n);
  std::string out;
  out.reserve(in.size());
  char line[64];
  long cases = 0;
  for (size_t pos = 0; pos < in.size();) {
    size_t eol = pos;
    while (eol < in.size() && in[eol] != '\n') ++eol;
    const char kind = in[pos];
    if (eol - pos < 4 || in[pos + 1] != '\t') { fprintf(stderr, "bad line at byte %zu\n", pos); return 2; }
    size_t t2 = pos + 2;
    while (t2 < eol && in[t2] != '\t') ++t2;
    if (t2 >= eol) { fprintf(stderr, "bad line at byte %zu\n", pos); return 2; }
    const std::string spec(in.begin() + pos + 2, in.begin() + t2);
    const size_t len = eol - (t2 + 1);
    uint8_t* text = new uint8_t[len];                 // exact size: ASan sees one byte past
    memcpy(text, in.data() + t2 + 1, len);
    bool ok = true;
    int64_t v = 0;
    if (kind == 'T') {
      ok = parse_timestamp(text, text + len, &v);
    } else if (kind == 'C') {
      int sk, ss, dk, ds, dp;
      if (sscanf(spec.c_str(), "%d,%d,%d,%d,%d", &sk, &ss, &dk, &ds, &dp) != 5) { fprintf(stderr, "bad spec\n"); return 2; }
      const CastPlan plan = make_cast_plan(ss, dk == kCastDec, ds, dp);
      __int128 iv = 0;
      uint64_t bits = 0;
      if (sk == kCastF32 || sk == kCastF64) bits = strtoull(std::string((char*)text, len).c_str(), nullptr, 16);
      else iv = read_i128((const char*)text, len);
      switch (dk) {
        case kCastI8: ok = to_int<int8_t>(sk, iv, bits, plan, &v); break;
        case kCastI16: ok = to_int<int16_t>(sk, iv, bits, plan, &v); break;
        case kCastI32: ok = to_int<int32_t>(sk, iv, bits, plan, &v); break;
        case kCastI64: ok = to_int<int64_t>(sk, iv, bits, plan, &v); break;
        default: ok = to_dec(sk, iv, bits, plan, &v);
      }
    } else {
      fprintf(stderr, "unknown kind %c\n", kind);
      return 2;
    }
    snprintf(line, sizeof line, "ok\t%" PRId64 "\n", v);
    out += ok ? line : "err\n";
    delete[] text;
    ++cases;
    pos = eol + 1;
  }
  fwrite(out.data(), 1, out.size(), stdout);
  fprintf(stderr, "trycast_host: %ld cases, no sanitizer report\n", cases);
  return 0;
}
