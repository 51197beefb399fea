// Stand-alone sanitizer driver for the device routines of binary.hip (hex and base64 validators and
// writers, the UTF-8 automaton) and the blake2 compressors of digest.hip, compiled as plain C++ (one
// "thread" after another) under ASan / UBSan. Every buffer has its exact size, so a read or write one
// byte outside a row, an output or a flag array is a report. The expected values come from a table
// that tests/test_binary_host.py writes from Python's binascii / base64 / hashlib / bytes.decode:
//   R <hex of the bytes> <base64> <blake2b> <blake2s> <1 if valid UTF-8>     ("-" = empty)
//   XH <hex of a text hex-decode must reject>      XB <... base64-decode must reject>
//   VB <hex of a base64 text> <hex of its bytes>
// Kernels that stage offsets in LDS run with blockDim.x == 1 (the shim's barrier is a no-op).
#include "common.h"
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <vector>
#include "binary.inc"
#include "digest.inc"
using namespace igloo::kern;
typedef std::vector<uint8_t> Bytes;
struct Col { int64_t* off; uint8_t* data; uint8_t* valid; int64_t n, nbytes; };
// rows behind `lead` junk bytes (offsets do not start at 0); valid: 0 = NULL, bytes kept underneath
static Col make(const std::vector<Bytes>& v, const std::vector<int>* ok = nullptr, int64_t lead = 0) {
  Col c; c.n = (int64_t)v.size(); c.off = new int64_t[v.size() + 1]; int64_t t = lead; c.off[0] = lead;
  for (size_t i = 0; i < v.size(); ++i) { t += v[i].size(); c.off[i + 1] = t; }
  c.nbytes = t; c.data = new uint8_t[t]; memset(c.data, '#', lead); t = lead;    // exact size: ASan sees one byte past
  for (auto& s : v) { if (!s.empty()) memcpy(c.data + t, s.data(), s.size()); t += s.size(); }
  c.valid = nullptr;
  if (ok) { c.valid = new uint8_t[v.size()]; for (size_t i = 0; i < v.size(); ++i) c.valid[i] = (uint8_t)(*ok)[i]; }
  return c;
}
static void drop(Col& c) { delete[] c.off; delete[] c.data; delete[] c.valid; }
static Bytes unhex(const std::string& h) {
  Bytes o; if (h == "-") return o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((uint8_t)strtol(h.substr(i, 2).c_str(), nullptr, 16));
  return o;
}
static Bytes text(const std::string& s) { return s == "-" ? Bytes() : Bytes(s.begin(), s.end()); }
template <class F> static void run_grid(unsigned gd, unsigned bd, F f) {
  gridDim.x = gd; blockDim.x = bd;
  for (unsigned b = 0; b < gd; ++b) for (unsigned t = 0; t < bd; ++t) { blockIdx.x = b; threadIdx.x = t; f(); }
}
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("MISMATCH " __VA_ARGS__); printf("\n"); if (++fails > 20) exit(1); } } while (0)

static std::vector<int64_t> scan(const int64_t* lens, int64_t n) {
  std::vector<int64_t> o(n + 1, 0); for (int64_t i = 0; i < n; ++i) o[i + 1] = o[i] + lens[i]; return o;
}
// the smallest bad row the validators report (n = none); hex also says whether NULL rows hold bytes
static int64_t hex_bad(const Col& c, bool* null_bytes = nullptr) {
  unsigned long long err[2] = {(unsigned long long)c.n, 0};
  run_grid(3, 256, [&] { hex_validate_kernel(c.off, c.data, c.valid, c.n, err); });
  if (null_bytes) *null_bytes = err[1] != 0;
  return (int64_t)err[0];
}
static int64_t b64_bad(const Col& c, std::vector<int64_t>& lens) {
  unsigned long long err[1] = {(unsigned long long)c.n};
  lens.assign(std::max<int64_t>(c.n, 1), -7);
  run_grid(3, 256, [&] { b64_dec_lengths_kernel(c.off, c.data, c.valid, c.n, lens.data(), err); });
  return (int64_t)err[0];
}
// encode or decode the column through the cooperative writer; out has exactly the scanned size
static Bytes b64_run(bool enc, const Col& c, const std::vector<int64_t>& ooff) {
  const int64_t total = ooff[c.n];
  uint8_t* out = new uint8_t[total];
  for (unsigned gd : {1u, 3u}) {
    memset(out, 0, total);
    if (enc) run_grid(gd, 1, [&] { b64_write_kernel<true>(c.off, c.data, ooff.data(), c.n, total, out); });
    else run_grid(gd, 1, [&] { b64_write_kernel<false>(c.off, c.data, ooff.data(), c.n, total, out); });
  }
  if (total > 9) {       // an output smaller than the offsets say (a stale size): nothing is written past it
    uint8_t* cut = new uint8_t[total - 9];
    if (enc) run_grid(2, 1, [&] { b64_write_kernel<true>(c.off, c.data, ooff.data(), c.n, total - 9, cut); });
    else run_grid(2, 1, [&] { b64_write_kernel<false>(c.off, c.data, ooff.data(), c.n, total - 9, cut); });
    if (memcmp(cut, out, total - 9) != 0) { printf("MISMATCH clipped base64 output\n"); ++fails; }
    delete[] cut;
  }
  Bytes r(out, out + total); delete[] out; return r;
}

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: binary_host <table>\n"); return 2; }
  std::ifstream in(argv[1]); std::string line;
  std::vector<Bytes> rows, b64s, xh, xb, vb_text, vb_bytes; std::vector<std::string> b2b, b2s; std::vector<int> u8;
  while (std::getline(in, line)) {
    std::istringstream ls(line); std::string k, a, b, c, d, e; ls >> k >> a >> b >> c >> d >> e;
    if (k == "R") { rows.push_back(unhex(a)); b64s.push_back(text(b)); b2b.push_back(c); b2s.push_back(d); u8.push_back(e == "1"); }
    else if (k == "XH") xh.push_back(unhex(a));
    else if (k == "XB") xb.push_back(unhex(a));
    else if (k == "VB") { vb_text.push_back(unhex(a)); vb_bytes.push_back(unhex(b)); }
  }
  const int64_t n = (int64_t)rows.size();
  if (n == 0) { printf("empty table\n"); return 2; }
  long checked = 0;
  for (int64_t lead : {(int64_t)0, (int64_t)5}) {        // offsets from 0, and a sliced column
    Col c = make(rows, nullptr, lead);
    // ---- hex encode: the whole buffer (the junk in front included), offsets double
    uint8_t* hx = new uint8_t[2 * c.nbytes];
    run_grid(2, 256, [&] { hex_encode_kernel(c.data, c.nbytes, hx); });
    static const char* dg = "0123456789abcdef";
    for (int64_t k = 0; k < c.nbytes; ++k, ++checked)
      CHECK(hx[2 * k] == dg[c.data[k] >> 4] && hx[2 * k + 1] == dg[c.data[k] & 15], "hex encode byte %ld", (long)k);
    // ---- hex decode of that text (as a column with doubled offsets): validates, gives the bytes back
    Col h; h.n = n; h.nbytes = 2 * c.nbytes; h.data = hx; h.valid = nullptr; h.off = new int64_t[n + 1];
    for (int64_t i = 0; i <= n; ++i) h.off[i] = 2 * c.off[i];
    CHECK(hex_bad(h) == n, "hex text rejected (lead %ld)", (long)lead);
    const int64_t nout = (h.off[n] - h.off[0]) / 2;
    uint8_t* back = new uint8_t[nout];
    run_grid(2, 256, [&] { hex_decode_kernel(h.off, n, h.data, nout, back); });
    if (nout > 9) {      // a smaller output than the offsets say: nothing is written past it
      uint8_t* cut = new uint8_t[nout - 9];
      run_grid(2, 256, [&] { hex_decode_kernel(h.off, n, h.data, nout - 9, cut); });
      CHECK(memcmp(cut, back, nout - 9) == 0, "clipped hex decode");
      delete[] cut;
    }
    CHECK(nout == c.nbytes - lead && memcmp(back, c.data + lead, nout) == 0, "hex decode round trip (lead %ld)", (long)lead);
    delete[] back; delete[] h.off; delete[] hx;
    // ---- base64 encode: lengths, scan, cooperative writer
    std::vector<int64_t> lens(n);
    run_grid(2, 256, [&] { b64_enc_lengths_kernel(c.off, (const uint8_t*)nullptr, n, lens.data()); });
    std::vector<int64_t> ooff = scan(lens.data(), n);
    Bytes enc = b64_run(true, c, ooff);
    for (int64_t i = 0; i < n; ++i, ++checked) {
      Bytes got(enc.begin() + ooff[i], enc.begin() + ooff[i + 1]);
      CHECK(got == b64s[i], "base64 encode row %ld (lead %ld)", (long)i, (long)lead);
    }
    // ---- base64 decode of the expected texts: validates, lengths, bytes back
    Col e = make(b64s, nullptr, lead);
    std::vector<int64_t> dl;
    CHECK(b64_bad(e, dl) == n, "base64 text rejected (lead %ld)", (long)lead);
    std::vector<int64_t> doff = scan(dl.data(), n);
    Bytes dec = b64_run(false, e, doff);
    for (int64_t i = 0; i < n; ++i, ++checked) {
      Bytes got(dec.begin() + doff[i], dec.begin() + doff[i + 1]);
      CHECK(got == rows[i], "base64 decode row %ld (lead %ld)", (long)i, (long)lead);
    }
    drop(e);
    // ---- utf-8: the automaton per row, and the row kernel behind all-set and exact tile flags
    const int64_t tiles = (c.nbytes + kUtf8Tile - 1) / kUtf8Tile;
    uint8_t* flags = new uint8_t[std::max<int64_t>(tiles, 1)];
    int64_t first_bad = n;
    for (int64_t i = 0; i < n; ++i, ++checked) {
      const bool ok = utf8_row_ok(c.data + c.off[i], c.off[i + 1] - c.off[i]);
      CHECK(ok == (u8[i] != 0), "utf8 row %ld", (long)i);
      if (!u8[i] && first_bad == n) first_bad = i;
    }
    for (int exact = 0; exact < 2; ++exact) {
      for (int64_t t = 0; t < tiles; ++t) {
        flags[t] = 1;
        if (exact) {
          // the tile kernel's per-lane share (its 16-byte load and its bytewise tail at the end of the
          // exact-size buffer), OR-ed over the block's lanes as the device's block vote does
          flags[t] = 0;
          for (int lane = 0; lane < kBlock; ++lane) flags[t] |= (uint8_t)utf8_lane_high(c.data, c.nbytes, t * kUtf8Tile + 16 * lane);
          uint8_t want = 0;
          for (int64_t j = t * kUtf8Tile; j < std::min<int64_t>(c.nbytes, (t + 1) * kUtf8Tile); ++j) want |= c.data[j] >> 7;
          CHECK(flags[t] == want, "utf8 tile flag %ld", (long)t);
        }
      }
      unsigned long long err[1] = {(unsigned long long)n};
      run_grid(2, 256, [&] { utf8_validate_kernel(c.off, c.data, (const uint8_t*)nullptr, n, flags, err); });
      CHECK((int64_t)err[0] == first_bad, "utf8 first bad row %ld want %ld", (long)err[0], (long)first_bad);
    }
    delete[] flags;
    // ---- blake2b / blake2s through their kernels
    uint8_t* d = new uint8_t[n * 128];
    run_grid(2, 256, [&] { blake2_hex_kernel<uint64_t>(c.off, c.data, n, d); });
    for (int64_t i = 0; i < n; ++i, ++checked) CHECK(std::string((char*)d + 128 * i, 128) == b2b[i], "blake2b row %ld", (long)i);
    run_grid(2, 256, [&] { blake2_hex_kernel<uint32_t>(c.off, c.data, n, d); });
    for (int64_t i = 0; i < n; ++i, ++checked) CHECK(std::string((char*)d + 64 * i, 64) == b2s[i], "blake2s row %ld", (long)i);
    delete[] d;
    drop(c);
  }
  // ---- rejected inputs: first, last of a block, alone, and under a NULL (never reported)
  const Bytes good_hex = {'0', 'a'}, good_b64 = {'Q', 'Q'};
  for (int kind = 0; kind < 2; ++kind) {
    const auto& bads = kind ? xb : xh; const Bytes& good = kind ? good_b64 : good_hex;
    for (const Bytes& bad : bads) {
      struct P { std::vector<Bytes> v; std::vector<int> ok; int64_t want; };
      std::vector<P> ps;
      { P p; p.v.assign(300, good); p.v[0] = bad; p.ok.assign(300, 1); p.want = 0; ps.push_back(p); }
      { P p; p.v.assign(300, good); p.v[255] = bad; p.ok.assign(300, 1); p.want = 255; ps.push_back(p); }
      { P p; p.v = {bad}; p.ok = {1}; p.want = 0; ps.push_back(p); }
      { P p; p.v = {good, bad, good}; p.ok = {1, 0, 1}; p.want = 3; ps.push_back(p); }
      { P p; p.v = {bad}; p.ok = {0}; p.want = 1; ps.push_back(p); }
      for (auto& p : ps) for (int64_t lead : {(int64_t)0, (int64_t)3}) {
        Col c = make(p.v, &p.ok, lead); std::vector<int64_t> dl;
        const int64_t got = kind ? b64_bad(c, dl) : hex_bad(c);
        CHECK(got == p.want, "%s reject: first bad row %ld want %ld (%zu rows)", kind ? "base64" : "hex", (long)got, (long)p.want, p.v.size());
        if (kind) for (size_t i = 0; i < p.v.size(); ++i) CHECK(!p.ok[i] ? dl[i] == 0 : true, "NULL row has a length");
        ++checked; drop(c);
      }
    }
  }
  // ---- accepted base64 spellings (padded and not) decode to their bytes
  {
    Col c = make(vb_text); std::vector<int64_t> dl;
    CHECK(b64_bad(c, dl) == c.n, "valid base64 rejected");
    std::vector<int64_t> doff = scan(dl.data(), c.n);
    Bytes dec = b64_run(false, c, doff);
    for (int64_t i = 0; i < c.n; ++i, ++checked)
      CHECK(Bytes(dec.begin() + doff[i], dec.begin() + doff[i + 1]) == vb_bytes[i], "base64 spelling %ld", (long)i);
    drop(c);
  }
  if (fails) { printf("%d mismatches\n", fails); return 1; }
  printf("ok: %ld checks equal the Python tables, no sanitizer report\n", checked);
  return 0;
}
