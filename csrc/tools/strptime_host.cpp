// Stand-alone sanitizer driver for the format-program parser: parse_by_program of
// csrc/kernels/strptime.h compiled as plain C++ under ASan / UBSan through the host shim
// (strpair_host_shim.h as common.h). Every text and every program is copied into a heap buffer
// of its exact size, so a read one byte outside either is an AddressSanitizer report; signed
// overflow is a UBSan report.
//
// stdin, one case per line:
//   program-hex <TAB> unit <TAB> text        -> ok <TAB> value, or "bad" where no format matches
//   program-hex <TAB> unit:b:e:nbytes <TAB> text
//        the kernel's row guard: the row is [b, e) of a buffer of nbytes bytes (the text); a row
//        that is negative, reversed or reaches past nbytes is "bad" and its bytes are not read
// The text is every byte after the second TAB up to the newline. Built and run by
// tests/test_strptime_host.py (no GPU).
#include "common.h"
#include <cinttypes>
#include <cstdio>
#include <vector>
#include "strptime.h"
using namespace igloo::kern;

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

int main() {
  std::vector<char> in;
  char chunk[1 << 16];
  for (size_t n; (n = fread(chunk, 1, sizeof chunk, stdin)) > 0;) in.insert(in.end(), chunk, chunk + n);
  std::string out;
  out.reserve(in.size() / 4);
  char line[64];
  long cases = 0;
  for (size_t pos = 0; pos < in.size();) {
    size_t eol = pos;
    while (eol < in.size() && in[eol] != '\n') ++eol;
    size_t t1 = pos;
    while (t1 < eol && in[t1] != '\t') ++t1;
    size_t t2 = t1 + 1;
    while (t2 < eol && in[t2] != '\t') ++t2;
    if (t1 >= eol || t2 >= eol || (t1 - pos) % 2) { fprintf(stderr, "bad line at byte %zu\n", pos); return 2; }
    const size_t plen = (t1 - pos) / 2;
    uint8_t* prog = new uint8_t[plen];                // exact size: ASan sees one byte past
    for (size_t k = 0; k < plen; ++k) {
      const int hi = hexval(in[pos + 2 * k]), lo = hexval(in[pos + 2 * k + 1]);
      if (hi < 0 || lo < 0) { fprintf(stderr, "bad program at byte %zu\n", pos); return 2; }
      prog[k] = (uint8_t)(hi * 16 + lo);
    }
    const std::string spec(in.begin() + t1 + 1, in.begin() + t2);
    const size_t len = eol - (t2 + 1);
    uint8_t* text = new uint8_t[len];
    memcpy(text, in.data() + t2 + 1, len);
    int unit = 0;
    long long b = 0, e = (long long)len, nbytes = (long long)len;
    const int got = sscanf(spec.c_str(), "%d:%lld:%lld:%lld", &unit, &b, &e, &nbytes);
    if (got != 1 && got != 4) { fprintf(stderr, "bad spec at byte %zu\n", pos); return 2; }
    int64_t v = 0;
    // the guard of strptime_kernel, then the element routine
    const bool ok = b >= 0 && e >= b && e <= nbytes && nbytes <= (long long)len &&
                    parse_by_program(text + b, text + e, prog, (int)plen, unit, &v);
    snprintf(line, sizeof line, "ok\t%" PRId64 "\n", v);
    out += ok ? line : "bad\n";
    delete[] text;
    delete[] prog;
    ++cases;
    pos = eol + 1;
  }
  fwrite(out.data(), 1, out.size(), stdout);
  fprintf(stderr, "strptime_host: %ld cases, no sanitizer report\n", cases);
  return 0;
}
