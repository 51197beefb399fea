// Stand-alone sanitizer driver for the text <-> value routines of csrc/kernels/textparse.h
// (parse_int, parse_decimal, parse_f64, parse_date, format_fixed, format_date), compiled as
// plain C++ under ASan / UBSan. Every input is copied into a heap buffer of its exact size and
// every output is written into one of the exact size the routine announced, so a read or write
// one byte outside either is an AddressSanitizer report; signed overflow is a UBSan report.
//
// stdin:  kind <TAB> scale <TAB> text        one case per line, text may be empty
//   f  parse_f64         -> ok <TAB> the double's bits, 16 hex digits
//   i  parse_int         -> ok <TAB> the int64
//   d  parse_decimal     -> ok <TAB> the scaled int64
//   t  parse_date        -> ok <TAB> days since 1970-01-01
//   F  format_fixed      -> ok <TAB> text   (text: the int64 value, scale: its scale)
//   D  format_date       -> ok <TAB> text   (text: the date32 value)
// A rejected input prints "err". Built and run by tests/test_textparse_host.py (no GPU).
#include "common.h"
#include <cinttypes>
#include <cstdio>
#include <vector>
#include "textparse.h"
using namespace igloo::kern;

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
    const int scale = atoi(std::string(in.begin() + pos + 2, in.begin() + t2).c_str());
    const size_t len = eol - (t2 + 1);
    uint8_t* text = new uint8_t[len];                 // exact size: ASan sees one byte past
    memcpy(text, in.data() + t2 + 1, len);
    bool ok = true;
    switch (kind) {
      case 'f': {
        double v = 0;
        ok = parse_f64(text, text + len, &v);
        uint64_t b;
        memcpy(&b, &v, 8);
        snprintf(line, sizeof line, "ok\t%016" PRIx64 "\n", b);
        break;
      }
      case 'i': {
        int64_t v = 0;
        ok = parse_int(text, text + len, &v);
        snprintf(line, sizeof line, "ok\t%" PRId64 "\n", v);
        break;
      }
      case 'd': {
        int64_t v = 0;
        ok = parse_decimal(text, text + len, scale, &v);
        snprintf(line, sizeof line, "ok\t%" PRId64 "\n", v);
        break;
      }
      case 't': {
        int32_t v = 0;
        ok = parse_date(text, text + len, &v);
        snprintf(line, sizeof line, "ok\t%d\n", v);
        break;
      }
      case 'F':
      case 'D': {
        const long long v = strtoll(std::string((char*)text, len).c_str(), nullptr, 10);
        const int n = kind == 'F' ? format_fixed(v, scale, nullptr) : format_date((int32_t)v, nullptr);
        uint8_t* o = new uint8_t[n];
        const int n2 = kind == 'F' ? format_fixed(v, scale, o) : format_date((int32_t)v, o);
        if (n2 != n) { fprintf(stderr, "length pass and write pass disagree\n"); return 3; }
        out += "ok\t";
        out.append((char*)o, n);
        out += "\n";
        line[0] = 0;
        delete[] o;
        break;
      }
      default:
        fprintf(stderr, "unknown kind %c\n", kind);
        return 2;
    }
    out += ok ? line : "err\n";
    delete[] text;
    ++cases;
    pos = eol + 1;
  }
  fwrite(out.data(), 1, out.size(), stdout);
  fprintf(stderr, "textparse_host: %ld cases, no sanitizer report\n", cases);
  return 0;
}
