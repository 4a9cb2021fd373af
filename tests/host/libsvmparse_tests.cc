// libsvmparse_tests — the device libsvm path against the host reader (the yardstick is
// difacto_amd/host/reader.cc: ParseLibSVM, GatherRows, BatchReader, TextReader).  Every
// comparison is exact (bytes), values and labels bit for bit.
//
//   GPU modes
//     parse FILE        dfx_parse_libsvm == ParseLibSVM with needs_host == 0: FILE (rcv1-100)
//                       whole and through an unaligned pointer; one row, a row with no feature,
//                       "1\n", nbytes 0 and 2^31; label / id / ':' / value ending one before, at
//                       and one after a 16-byte thread boundary and a 4 KiB tile boundary; a line
//                       spanning three tiles (tiles with no newline); a 64-byte token (clean) and
//                       a 65-byte one (flagged); runs of 1-5 blanks and tabs, leading and
//                       trailing; the strtof edge strings as labels and values; ids of 19 / 20 /
//                       30 digits; a text of more tiles than one pass of the tile-totals scan
//                       covers (1024 tiles of 4 KiB); capacities one too small (DFX_ERR_CAPACITY,
//                       needed counts, guard words intact); the row flags
//     fallback          CRLF, blank line, inf, nan, 0x1p3, 1e, "3:" + blank, abc, a 25-digit
//                       value, q = 28, a signed id, an unterminated last line: none of these is
//                       required to stay on the device; each is flagged (needs_host) or exactly
//                       ParseLibSVM's output.  ParseLibSVM does not terminate on "1e" and "abc"
//                       (strtoull makes no progress), so for those the flag is required.
//     gather            dfx_gather_rows_valued == GatherRows: range, permuted list, gaps, n = 0,
//                       r0 > 0, zero-length rows, value NULL on either side, flags carried
//     batches FILE DIR  DeviceBatchReader("libsvm") == BatchReader batch by batch, valued-or-not
//                       included (batch 257, 64 KB chunks, shuffle 0 / 3, neg_sampling 1 / 0.7,
//                       parts 0/1 and 1/2), whole chunks as batches, a file whose long rows make
//                       the ring entry and the shuffle buffer grow mid-run, a flagged file
//     feedargs          the text feed's argument checks, on a Criteo and a libsvm feed (batch 4,
//                       shuffle buffer 8): values asked of or given to a Criteo feed, features
//                       without values on a libsvm feed, the shuffle buffer gathered onto
//                       itself and a gather with no batch begun are DFX_ERR_ARG with a message;
//                       a three-row chunk then goes text -> submit -> wait -> batch_begin ->
//                       gather -> batch_end and equals the host parser's block
//   CPU mode (no HIP call)
//     plan FILE         BatchPlanner's plan carried out with GatherRows and the row-flag
//                       mirroring == BatchReader, including which batches drop their values
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "../../difacto_amd/host/device_reader.h"
#include "../../difacto_amd/host/gpu_adapters.h"
#include "../../difacto_amd/host/reader.h"

using namespace difacto;

namespace {
int g_fail = 0;
#define EXPECT(cond, ...)                          \
  do {                                             \
    if (!(cond)) {                                 \
      ++g_fail;                                    \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                    \
      std::printf("\n");                           \
    }                                              \
  } while (0)

typedef RowBlockContainer<feaid_t> Block;

std::string ReadFile(const std::string& path) {
  std::ifstream in(path, std::ios::binary);
  return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

Block HostParse(const std::string& text) {
  Block b;
  ParseLibSVM(text.data(), text.data() + text.size(), &b);
  return b;
}

std::vector<uint8_t> HostFlags(const Block& b) {
  std::vector<uint8_t> f(b.Size(), 0);
  for (size_t r = 0; r < b.Size(); ++r)
    for (size_t k = b.offset[r]; k < b.offset[r + 1]; ++k) {
      uint32_t bits;
      std::memcpy(&bits, &b.value[k], 4);
      if (bits != 0x3f800000u) f[r] = 1;
    }
  return f;
}

// short valued rows: 0-4 features, %g values, some bare ids
std::string GenRows(int rows, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::string out;
  char buf[64];
  for (int r = 0; r < rows; ++r) {
    out += rng() % 3 ? "1" : "0";
    const int nnz = (int)(rng() % 5);
    for (int j = 0; j < nnz; ++j) {
      if (rng() % 4 == 0)
        std::snprintf(buf, sizeof buf, " %u", (unsigned)(rng() % 100000));
      else
        std::snprintf(buf, sizeof buf, " %u:%g", (unsigned)(rng() % 100000),
                      (double)(rng() % 100000) / 1000.0);
      out += buf;
    }
    out += '\n';
  }
  return out;
}

// the strings of tools/strtof_check.cc's edge list that are in the fast grammar
const char* const kEdges[] = {
    "16777217", "16777219", "33554434", "8388608.5", "8388609.5", "0.1", "1e-27",
    "9999999999999999999e27", "9999999999999999999e-27", "-0", "0e99", ".5", "5.", "+1", "1e+05",
    "1E-3", "1234567890123456789", "0000000000000000000000000000001", "3402823466385288598e20",
    "3402823567797336616e20", "3402823567797336617e20", "3402823567797336615e20",
    "340282350000e27", "340282360000e27", "1.0000001", "-1",
    "0.99999997019767761"};

// ---- device helpers ----------------------------------------------------------------------
const uint64_t kGuard = 0xdeadbeefcafef00dULL;
const int kGuardWords = 8;

struct Dev {
  dfx_ctx* c;
  void* p = nullptr;
  Dev(dfx_ctx* ctx, size_t bytes) : c(ctx) { DfxCheck(dfx_malloc(c, &p, bytes), "dfx_malloc"); }
  ~Dev() { dfx_free(c, p); }
  void Up(const void* src, size_t bytes, size_t at = 0) {
    DfxCheck(dfx_memcpy(c, static_cast<char*>(p) + at, src, bytes, 0), "upload");
  }
  void Down(void* dst, size_t bytes, size_t at = 0) {
    DfxCheck(dfx_memcpy(c, dst, static_cast<char*>(p) + at, bytes, 1), "download");
  }
};

struct Parsed {
  int rc = 0;
  int64_t stat[4] = {0, 0, 0, 0};
  std::vector<uint64_t> offset, index;
  std::vector<float> value, label;
  std::vector<uint8_t> flag;
  bool guards_ok = true;
};

// dfx_parse_libsvm of text with the given capacities; guard words follow every output array
Parsed DeviceParse(dfx_ctx* c, const std::string& text, int64_t max_rows, int64_t max_nnz,
                   int misalign = 0) {
  Parsed out;
  const size_t G = kGuardWords * 8;
  Dev dtext(c, text.size() + 64), doff(c, (max_rows + 1) * 8 + G), didx(c, max_nnz * 8 + G),
      dval(c, max_nnz * 4 + G), dlab(c, max_rows * 4 + G), dflag(c, max_rows + G), dstat(c, 32);
  if (!text.empty()) dtext.Up(text.data(), text.size(), misalign);
  const std::vector<uint64_t> g(kGuardWords, kGuard);
  doff.Up(g.data(), G, (max_rows + 1) * 8);
  didx.Up(g.data(), G, max_nnz * 8);
  dval.Up(g.data(), G, max_nnz * 4);
  dlab.Up(g.data(), G, max_rows * 4);
  dflag.Up(g.data(), G, max_rows);
  DfxCheck(dfx_sync(c), "dfx_sync");
  out.rc = dfx_parse_libsvm(c, static_cast<char*>(dtext.p) + misalign, (int64_t)text.size(),
                            max_rows, max_nnz, static_cast<uint64_t*>(doff.p),
                            static_cast<uint64_t*>(didx.p), static_cast<float*>(dval.p),
                            static_cast<float*>(dlab.p), static_cast<uint8_t*>(dflag.p),
                            static_cast<int64_t*>(dstat.p));
  if (out.rc != DFX_OK) return out;
  out.rc = dfx_parse_criteo_wait(c, static_cast<int64_t*>(dstat.p), out.stat);
  std::vector<uint64_t> g1(kGuardWords), g2(kGuardWords), g3(kGuardWords), g4(kGuardWords),
      g5(kGuardWords);
  doff.Down(g1.data(), G, (max_rows + 1) * 8);
  didx.Down(g2.data(), G, max_nnz * 8);
  dval.Down(g3.data(), G, max_nnz * 4);
  dlab.Down(g4.data(), G, max_rows * 4);
  dflag.Down(g5.data(), G, max_rows);
  out.guards_ok = g1 == g && g2 == g && g3 == g && g4 == g && g5 == g;
  if (out.rc == DFX_OK && !out.stat[2]) {
    const int64_t rows = out.stat[0], nnz = out.stat[1];
    out.offset.resize(rows + 1);
    out.index.resize(nnz);
    out.value.resize(nnz);
    out.label.resize(rows);
    out.flag.resize(rows);
    doff.Down(out.offset.data(), (rows + 1) * 8);
    if (nnz) didx.Down(out.index.data(), nnz * 8);
    if (nnz) dval.Down(out.value.data(), nnz * 4);
    if (rows) dlab.Down(out.label.data(), rows * 4);
    if (rows) dflag.Down(out.flag.data(), rows);
  }
  return out;
}

// offsets, ids, values and labels byte for byte (values: want.value empty means none to compare)
bool SameBlock(const Block& want, const uint64_t* off, const uint64_t* idx, const float* val,
               const float* lab, size_t rows, size_t nnz) {
  if (want.Size() != rows || want.index.size() != nnz) return false;
  for (size_t i = 0; i <= rows; ++i)
    if (want.offset[i] != off[i]) return false;
  if (nnz && std::memcmp(want.index.data(), idx, nnz * 8) != 0) return false;
  if (nnz && val && std::memcmp(want.value.data(), val, nnz * 4) != 0) return false;
  if (rows && std::memcmp(want.label.data(), lab, rows * 4) != 0) return false;
  return true;
}

bool SameParsed(const Block& want, const Parsed& got) {
  return SameBlock(want, got.offset.data(), got.index.data(), got.value.data(), got.label.data(),
                   got.label.size(), got.index.size()) &&
         got.flag == HostFlags(want);
}

// exact capacities: the device must match the host, unflagged, and stay inside them
bool CheckClean(dfx_ctx* c, const std::string& name, const std::string& text, int misalign = 0,
                bool quiet = false) {
  const int before = g_fail;
  const Block want = HostParse(text);
  const Parsed got =
      DeviceParse(c, text, (int64_t)want.Size(), (int64_t)want.index.size(), misalign);
  EXPECT(got.rc == DFX_OK, "%s: status %d (%s)", name.c_str(), got.rc, dfx_last_error());
  EXPECT(got.guards_ok, "%s: guard words overwritten", name.c_str());
  EXPECT(got.stat[2] == 0, "%s: needs_host raised", name.c_str());
  EXPECT(got.stat[3] == 0, "%s: overflow raised", name.c_str());
  if (got.rc == DFX_OK && !got.stat[2]) {
    EXPECT((size_t)got.stat[0] == want.Size() && (size_t)got.stat[1] == want.index.size(),
           "%s: %lld rows %lld features, host %zu %zu", name.c_str(), (long long)got.stat[0],
           (long long)got.stat[1], want.Size(), want.index.size());
    EXPECT(SameParsed(want, got), "%s: device block != ParseLibSVM", name.c_str());
  }
  if (!quiet)
    std::printf("parse %s: %zu bytes, %zu rows, %zu features ok\n", name.c_str(), text.size(),
                want.Size(), want.index.size());
  return g_fail == before;
}

// `line` placed so that its byte `at` lands on text position `pos`: 6-byte filler rows, then
// up to 5 blanks in front of the line's label
std::string PlaceAt(const std::string& line, size_t at, size_t pos) {
  std::string out;
  if (pos < at) return line;
  size_t pad = pos - at;
  while (pad >= 6) {
    out += "0 7:2\n";
    pad -= 6;
  }
  out.append(pad, ' ');
  return out + line + "1 9:3\n";
}

int ModeParse(dfx_ctx* c, const std::string& rcv1) {
  const std::string file = ReadFile(rcv1);
  EXPECT(!file.empty(), "cannot read %s", rcv1.c_str());
  CheckClean(c, "(a) rcv1-100", file);
  CheckClean(c, "(a) rcv1-100, unaligned text", file, 3);
  CheckClean(c, "(b) one row", "1 3:0.5 7 9:2\n");
  CheckClean(c, "(b) a row with no feature", "1 3:0.5\n0\n-1 4\n");
  CheckClean(c, "(b) \"1\\n\" alone", "1\n");
  {
    const Parsed got = DeviceParse(c, "", 4, 4);
    EXPECT(got.rc == DFX_OK && got.stat[0] == 0 && got.stat[1] == 0 && got.stat[2] == 0 &&
               got.stat[3] == 0 && got.guards_ok && got.offset.size() == 1 && got.offset[0] == 0,
           "(b) nbytes = 0");
    Dev d(c, 64);
    const int rc = dfx_parse_libsvm(c, static_cast<char*>(d.p), 1ll << 31, 1, 1,
                                    static_cast<uint64_t*>(d.p), static_cast<uint64_t*>(d.p),
                                    static_cast<float*>(d.p), static_cast<float*>(d.p),
                                    static_cast<uint8_t*>(d.p), static_cast<int64_t*>(d.p));
    EXPECT(rc == DFX_ERR_ARG, "nbytes = 2^31: status %d", rc);
    std::printf("parse (b) nbytes 0 / 2^31 ok\n");
  }
  {  // (c) every part of a feature on the thread and tile boundaries
    const std::string line = "12.5 345:0.25 77\n";
    const struct {
      const char* what;
      size_t at;
    } parts[] = {{"label", 3}, {"id", 7}, {"':'", 8}, {"value", 12}, {"bare id", 15}, {"'\\n'", 16}};
    int n = 0;
    for (size_t bound : {(size_t)16, (size_t)4096, (size_t)8192})
      for (const auto& p : parts)
        for (int d = -1; d <= 1; ++d) {
          char name[96];
          std::snprintf(name, sizeof name, "(c) %s ends at %zu%+d", p.what, bound - 1, d);
          CheckClean(c, name, PlaceAt(line, p.at, bound - 1 + d), 0, true);
          ++n;
        }
    std::printf("parse (c) %d boundary placements ok\n", n);
  }
  {  // (d) a line spanning three tiles: the tiles between have no newline
    std::string t = "1 2:3\n1";
    char buf[32];
    for (int j = 0; j < 1500; ++j) {
      std::snprintf(buf, sizeof buf, " %d:%g", 1000 + j, 0.5 + j);
      t += buf;
    }
    t += "\n0 5:1\n";
    EXPECT(t.size() > 3 * 4096, "(d) too short");
    CheckClean(c, "(d) a line spanning three tiles", t);
  }
  {  // (e) the token cap: 64 bytes parse, 65 are handed back
    const std::string id40(40, '9'), val = "0.000000000000000000125";
    const std::string t64 = id40 + ":" + val, t65 = "9" + t64;
    EXPECT(t64.size() == 64, "(e) token length %zu", t64.size());
    CheckClean(c, "(e) a 64-byte token", "1 5:2 " + t64 + " 3\n0 1\n");
    const std::string text = GenRows(300, 11) + "1 5:2 " + t65 + " 3\n" + GenRows(300, 12);
    const Parsed got = DeviceParse(c, text, 700, 4000);
    EXPECT(got.rc == DFX_OK && got.guards_ok && got.stat[2] == 1,
           "(e) a 65-byte token: status %d needs_host %lld", got.rc, (long long)got.stat[2]);
    std::printf("parse (e) a 65-byte token: needs_host ok\n");
  }
  CheckClean(c, "(f) runs of blanks and tabs",
             "1 2:3  4:5   6\t7:8\t\t9 \t 10:1\t \t \t11\n"
             "  0 1:2\n\t1 3\n \t \t 0     5:6     \n1 2 \n0\t\n1 \t\n     1\n0 1:2\t\t\t\t\t\n");
  {  // (g) the strtof edges as labels and as values
    std::string t;
    int k = 0;
    std::vector<std::string> edges(std::begin(kEdges), std::end(kEdges));
    edges.push_back("0." + std::string(26, '0') + "1");  // q = -27
    edges.push_back(std::string(40, '0') + "1");
    for (const std::string& e : edges) t += e + " " + std::to_string(++k) + ":" + e + "\n";
    CheckClean(c, "(g) strtof edges as labels and values", t);
  }
  CheckClean(c, "(h) ids of 19 / 20 / 30 digits",
             "1 1234567890123456789:2 9999999999999999999 10000000000000000000:0.5\n"
             "0 18446744073709551615 18446744073709551616:3 18446744073709551614\n"
             "1 123456789012345678901234567890:1.5 000000000000000000000000000042 0:0\n");
  {  // (i) more tiles than one pass of k_scan_totals covers (1024 tiles of 4 KiB)
    const std::string t = GenRows(330000, 5);
    EXPECT(t.size() > 1100u * 4096u, "(i) only %zu bytes", t.size());
    CheckClean(c, "(i) more than 1024 tiles", t);
  }
  {  // (j) capacities one too small
    const std::string a = GenRows(3000, 6);
    const Block want = HostParse(a);
    const int64_t rows = want.Size(), nnz = want.index.size();
    for (int which = 0; which < 2; ++which) {
      const Parsed got = DeviceParse(c, a, rows - (which == 0), nnz - (which == 1));
      EXPECT(got.rc == DFX_ERR_CAPACITY, "(j) %s too small: status %d",
             which ? "max_nnz" : "max_rows", got.rc);
      EXPECT(got.stat[3] == 1 && got.stat[0] == rows && got.stat[1] == nnz,
             "(j) needed counts %lld %lld, host %lld %lld", (long long)got.stat[0],
             (long long)got.stat[1], (long long)rows, (long long)nnz);
      EXPECT(got.guards_ok, "(j) guard words overwritten");
    }
    std::printf("parse (j) capacity ok\n");
  }
  {  // (k) the row flags: only a value whose bits are not 1.0f's flags its row
    const std::string t =
        "1 5 6 7\n0 5:1 6:1\n1 5:1.0 6:1.00\n0 5:1e0 6:+1 7:10e-1\n1 5:1.0000001\n0 5:-1\n1 5:1 6:2\n"
        "0\n1 5:0.99999997019767762\n";  // just above the tie below 1.0f: rounds to 1.0f
    const Block want = HostParse(t);
    const std::vector<uint8_t> wantf = {0, 0, 0, 0, 1, 1, 1, 0, 0};
    EXPECT(HostFlags(want) == wantf, "(k) the host's flags are not the expected ones");
    const Parsed got = DeviceParse(c, t, want.Size(), want.index.size());
    EXPECT(got.rc == DFX_OK && !got.stat[2] && got.flag == wantf, "(k) row flags differ");
    CheckClean(c, "(k) row flags", t);
    const Parsed nan = DeviceParse(c, "1 5:1\n0 6:nan\n", 2, 2);
    EXPECT(nan.rc == DFX_OK && nan.stat[2] == 1, "(k) :nan is not handed back");
  }
  return 0;
}

int ModeFallback(dfx_ctx* c) {
  const std::string body = GenRows(50, 4);
  std::string crlf;
  for (char ch : body) {
    if (ch == '\n') crlf += '\r';
    crlf += ch;
  }
  // host: 0 = ParseLibSVM does not terminate on the form (strtoull makes no progress on a
  // non-digit): the device must flag it and the host is not called
  struct Case {
    const char* name;
    std::string text;
    int host;
  } cases[] = {
      {"CRLF", crlf, 1},
      {"blank line", body.substr(0, body.find('\n') + 1) + "\n" + body, 1},
      {"blank-only line", body + " \t \n" + body, 1},
      {"leading blank line", "\n" + body, 1},
      {"value inf", body + "1 2:inf 3:1\n" + body, 1},
      {"value nan", body + "1 2:nan\n", 1},
      {"value 0x1p3", body + "1 2:0x1p3\n" + body, 1},
      {"label 0x10", body + "0x10 2:1\n", 1},
      {"value 1e", body + "1 2:1e\n" + body, 0},
      {"\"3:\" then a blank", body + "1 3: 4:1\n" + body, 1},
      {"feature abc", body + "1 abc\n" + body, 0},
      {"label abc", "abc 1:2\n" + body, 0},
      {"a 25-digit value", body + "1 2:1234567890123456789012345\n" + body, 1},
      {"q = 28", body + "1 2:1e28 3:1e-28\n" + body, 1},
      {"a signed id", body + "1 +5:2 -6\n" + body, 1},
      {"\":5\"", body + "1 :5\n" + body, 1},
      {"unterminated last line", body.substr(0, body.size() - 1), 1},
  };
  for (const Case& cs : cases) {
    int64_t lines = 1, blanks = 1;
    for (char ch : cs.text) {
      lines += ch == '\n';
      blanks += ch == ' ' || ch == '\t';
    }
    const Parsed got = DeviceParse(c, cs.text, lines, blanks);
    EXPECT(got.rc == DFX_OK && got.guards_ok, "%s: status %d guards %d", cs.name, got.rc,
           (int)got.guards_ok);
    if (got.rc != DFX_OK) continue;
    if (!cs.host) {
      EXPECT(got.stat[2] == 1, "%s: not handed back", cs.name);
    } else if (!got.stat[2]) {
      EXPECT(SameParsed(HostParse(cs.text), got), "%s: not flagged and != ParseLibSVM", cs.name);
    }
    std::printf("fallback %s: %s\n", cs.name, got.stat[2] ? "needs_host" : "equal");
  }
  return 0;
}

// ---- gather ------------------------------------------------------------------------------
int ModeGather(dfx_ctx* c) {
  const Block src = HostParse(GenRows(500, 6) + "1\n0\n1\n" + GenRows(300, 7));
  Block bin = src;  // the same rows as binary data
  bin.value.clear();
  const std::vector<uint8_t> sflag = HostFlags(src);
  const size_t R = src.Size(), N = src.index.size();
  Dev soff(c, (R + 1) * 8), sidx(c, N * 8), sval(c, N * 4), slab(c, R * 4), sflg(c, R);
  soff.Up(src.offset.data(), (R + 1) * 8);
  sidx.Up(src.index.data(), N * 8);
  sval.Up(src.value.data(), N * 4);
  slab.Up(src.label.data(), R * 4);
  sflg.Up(sflag.data(), R);
  const size_t cap_rows = 3 * R, cap_nnz = 3 * N;
  Dev doff(c, (cap_rows + 1) * 8), didx(c, cap_nnz * 8), dval(c, cap_nnz * 4),
      dlab(c, cap_rows * 4), dflg(c, cap_rows), drows(c, R * 4);
  Block want;
  std::vector<uint8_t> wantf;
  std::mt19937 rng(3);
  // with_src_val / with_dst_val: 0 passes NULL for that side's values
  auto step = [&](const char* name, const std::vector<size_t>* rows, size_t begin, size_t n,
                  bool with_src_val, bool with_dst_val) {
    std::vector<uint32_t> r32;
    if (rows) {
      for (size_t r : *rows) r32.push_back((uint32_t)r);
      if (n) drows.Up(r32.data(), n * 4);
    }
    const size_t r0 = want.Size();
    const int rc = dfx_gather_rows_valued(
        c, static_cast<uint64_t*>(soff.p), static_cast<uint64_t*>(sidx.p),
        with_src_val ? static_cast<float*>(sval.p) : nullptr, static_cast<float*>(slab.p),
        static_cast<uint8_t*>(sflg.p), rows ? static_cast<uint32_t*>(drows.p) : nullptr,
        (int64_t)begin, (int64_t)n, static_cast<uint64_t*>(doff.p),
        static_cast<uint64_t*>(didx.p), with_dst_val ? static_cast<float*>(dval.p) : nullptr,
        static_cast<float*>(dlab.p), static_cast<uint8_t*>(dflg.p), (int64_t)r0);
    EXPECT(rc == DFX_OK, "gather %s: status %d (%s)", name, rc, dfx_last_error());
    GatherRows(with_src_val ? src : bin, rows ? rows->data() : nullptr, begin, n, &want, 2);
    for (size_t i = 0; i < n; ++i) wantf.push_back(sflag[rows ? (*rows)[i] : begin + i]);
    const size_t rows_now = want.Size(), nnz_now = want.index.size();
    if (rows_now == 0) return;
    std::vector<uint64_t> off(rows_now + 1), idx(nnz_now);
    std::vector<float> lab(rows_now), val(nnz_now);
    std::vector<uint8_t> flg(rows_now);
    doff.Down(off.data(), (rows_now + 1) * 8);
    if (nnz_now) didx.Down(idx.data(), nnz_now * 8);
    if (nnz_now && with_dst_val) dval.Down(val.data(), nnz_now * 4);
    dlab.Down(lab.data(), rows_now * 4);
    dflg.Down(flg.data(), rows_now);
    EXPECT(!with_dst_val || want.value.size() == nnz_now, "gather %s: the host kept no values",
           name);
    EXPECT(SameBlock(want, off.data(), idx.data(), with_dst_val ? val.data() : nullptr,
                     lab.data(), rows_now, nnz_now),
           "gather %s: device block != GatherRows", name);
    EXPECT(flg == wantf, "gather %s: row flags not carried", name);
    std::printf("gather %s: %zu rows %zu features ok\n", name, rows_now, nnz_now);
  };
  std::vector<size_t> perm(R);
  for (size_t i = 0; i < R; ++i) perm[i] = i;
  std::shuffle(perm.begin(), perm.end(), rng);
  perm.resize(300);
  std::vector<size_t> gaps;
  for (size_t i = 2; i < R; i += 7) gaps.push_back(i);
  step("n = 0 into an empty destination", nullptr, 0, 0, true, true);
  step("range at r0 = 0", nullptr, 490, 80, true, true);  // spans the zero-length rows
  step("permuted list at r0 > 0", &perm, 0, perm.size(), true, true);
  step("list with gaps", &gaps, 0, gaps.size(), true, true);
  step("n = 0", &gaps, 0, 0, true, true);
  step("one row", nullptr, R - 1, 1, true, true);
  step("a binary source into valued rows (ones)", nullptr, 100, 257, false, true);
  step("range at r0 > 0", nullptr, 0, 257, true, true);
  // no destination values: the ids, labels and flags alone
  want = Block();
  wantf.clear();
  step("no destination values, r0 = 0", nullptr, 480, 60, true, false);
  step("no destination values, list at r0 > 0", &gaps, 0, gaps.size(), true, false);
  return 0;
}

// ---- batches -----------------------------------------------------------------------------
void JoinInput(dfx_ctx* c, Dev* dstat) {
  int64_t stat[4];
  DfxCheck(dfx_parse_criteo_wait(c, static_cast<int64_t*>(dstat->p), stat), "join input stream");
}

// want.value empty <=> the device batch has no values; else equal bytes
bool SameDeviceBatch(dfx_ctx* c, Dev* dstat, const Block& want, const dfx_batch& b) {
  JoinInput(c, dstat);
  if ((size_t)b.size != want.Size() || (size_t)b.nnz != want.index.size()) return false;
  if (want.value.empty() != (b.value == nullptr)) return false;
  std::vector<uint64_t> off(b.size + 1), idx(b.nnz);
  std::vector<float> lab(b.size), val(b.nnz);
  DfxCheck(dfx_memcpy(c, off.data(), b.offset, (b.size + 1) * 8, 1), "download");
  if (b.nnz) DfxCheck(dfx_memcpy(c, idx.data(), b.index, b.nnz * 8, 1), "download");
  if (b.nnz && b.value) DfxCheck(dfx_memcpy(c, val.data(), b.value, b.nnz * 4, 1), "download");
  DfxCheck(dfx_memcpy(c, lab.data(), b.label, b.size * 4, 1), "download");
  return SameBlock(want, off.data(), idx.data(), b.value ? val.data() : nullptr, lab.data(),
                   b.size, b.nnz);
}

struct Counts {
  size_t batches = 0, valued = 0, fallback = 0;
};

Counts CompareReaders(dfx_ctx* c, Dev* dstat, DeviceTextFeed* feed, const std::string& path,
                      int part, int nparts, size_t bs, size_t shuffle, float neg, size_t chunk) {
  BatchReader host(path, "libsvm", part, nparts, bs, bs * shuffle, neg, 4, chunk);
  DeviceBatchReader dev(feed, path, "libsvm", part, nparts, bs, bs * shuffle, neg, 4, chunk);
  Counts n;
  for (;;) {
    const bool a = host.Next(), b = dev.Next();
    EXPECT(a == b, "part %d/%d shuffle %zu neg %g: batch %zu: host %d device %d", part, nparts,
           shuffle, neg, n.batches, a, b);
    if (!a || !b) break;
    EXPECT(SameDeviceBatch(c, dstat, host.Value(), dev.Value()),
           "part %d/%d shuffle %zu neg %g: batch %zu differs (host valued %d, device %d)", part,
           nparts, shuffle, neg, n.batches, (int)!host.Value().value.empty(),
           (int)(dev.Value().value != nullptr));
    dev.Consumed();
    ++n.batches;
    n.valued += !host.Value().value.empty();
    if (g_fail > 5) break;
  }
  n.fallback = dev.FallbackChunks();
  return n;
}

int ModeBatches(dfx_ctx* c, const std::string& path, const std::string& dir) {
  Dev dstat(c, 32);
  const int64_t zero[4] = {0, 0, 0, 0};
  dstat.Up(zero, 32);
  const size_t bs = 257;
  DeviceTextFeed feed(c, bs, bs * 3, "libsvm");
  size_t valued = 0, binary = 0;
  for (size_t shuffle : {(size_t)0, (size_t)3})
    for (float neg : {1.f, 0.7f})
      for (int pp = 0; pp < 2; ++pp) {
        const Counts n =
            CompareReaders(c, &dstat, &feed, path, pp, pp + 1, bs, shuffle, neg, 64 << 10);
        std::printf("batches part %d/%d shuffle %zu neg %g: %zu batches (%zu valued) ok\n", pp,
                    pp + 1, shuffle, neg, n.batches, n.valued);
        EXPECT(n.batches > 3 && n.fallback == 0, "%zu batches, %zu fallback chunks", n.batches,
               n.fallback);
        valued += n.valued;
        binary += n.batches - n.valued;
      }
  EXPECT(valued > 0 && binary > 0, "%zu valued and %zu binary batches: both kinds must occur",
         valued, binary);
  {  // every chunk one batch (validation, prediction): valued iff a value is not 1.0f
    TextReader host(path, "libsvm", 0, 1, 64 << 10, 4);
    DeviceBatchReader dev(&feed, path, "libsvm", 0, 1, 0, 0, 1.f, 4, 64 << 10);
    size_t n = 0, nv = 0;
    for (;;) {
      bool a;
      do {
        a = host.Next();
      } while (a && host.Value().Size() == 0);
      const bool b = dev.Next();
      EXPECT(a == b, "whole chunks: chunk %zu: host %d device %d", n, a, b);
      if (!a || !b) break;
      Block want = host.Value();
      const std::vector<uint8_t> fl = HostFlags(want);
      if (std::find(fl.begin(), fl.end(), 1) == fl.end()) want.value.clear();
      EXPECT(SameDeviceBatch(c, &dstat, want, dev.Value()), "whole chunk %zu differs", n);
      EXPECT(std::memcmp(dev.HostLabels(), want.label.data(), want.Size() * 4) == 0,
             "whole chunk %zu: host labels differ", n);
      dev.Consumed();
      ++n;
      nv += !want.value.empty();
    }
    std::printf("batches whole chunks: %zu (%zu valued) ok\n", n, nv);
    EXPECT(n > 3 && nv > 0 && nv < n, "whole chunks: %zu, %zu valued", n, nv);
  }
  {  // rows of ~50,000 features among short ones: the ring entry and the shuffle buffer grow
    const std::string grow = dir + "/grow.libsvm";
    std::string out;
    std::mt19937_64 rng(21);
    char buf[48];
    for (int r = 0; r < 900; ++r) {
      if (r == 130 || r == 400 || r == 610) {
        out += "1";
        for (int j = 0; j < 50000 + r; ++j) {
          std::snprintf(buf, sizeof buf, " %d:%g", j * 3 + r, (double)((j * 7 + r) % 1000) / 8.0);
          out += buf;
        }
        out += '\n';
      } else {
        out += GenRows(1, 1000 + r);
      }
    }
    std::ofstream(grow, std::ios::binary) << out;
    for (size_t shuffle : {(size_t)0, (size_t)3}) {
      const Counts n = CompareReaders(c, &dstat, &feed, grow, 0, 1, bs, shuffle, 0.7f, 64 << 10);
      EXPECT(n.batches >= 3 && n.fallback == 0, "grow file: %zu batches", n.batches);
      std::printf("batches grow file shuffle %zu: %zu batches ok\n", shuffle, n.batches);
    }
  }
  {  // a file the device hands back: inf values, CRLF line ends, a hex label
    const std::string bad = dir + "/needs_host.libsvm";
    const std::string text = GenRows(9000, 9);
    std::string out;
    for (size_t i = 0, line = 0; i < text.size(); ++i) {
      if (text[i] == '\n') {
        ++line;
        if (line % 2000 == 0) out += " 77:inf";
        if (line % 3100 == 0) out += '\r';
      }
      out += text[i];
    }
    std::ofstream(bad, std::ios::binary) << out;
    const Counts n = CompareReaders(c, &dstat, &feed, bad, 0, 1, bs, 3, 0.7f, 16 << 10);
    // flagged and clean chunks in one run (about 14 chunks, 6 lines the device hands back)
    EXPECT(n.batches > 0 && n.fallback >= 3 && n.fallback <= 6,
           "needs_host file: %zu batches, %zu fallback chunks", n.batches, n.fallback);
    std::printf("batches needs_host file: %zu batches, %zu chunks parsed by the host ok\n",
                n.batches, n.fallback);
  }
  return 0;
}

// ---- the CPU mode ------------------------------------------------------------------------
bool SameHostBlock(const Block& a, const Block& b) {
  return a.Size() == b.Size() && a.offset == b.offset && a.index == b.index &&
         a.label.size() == b.label.size() && a.value.size() == b.value.size() &&
         (a.label.empty() ||
          std::memcmp(a.label.data(), b.label.data(), a.label.size() * 4) == 0) &&
         (a.value.empty() || std::memcmp(a.value.data(), b.value.data(), a.value.size() * 4) == 0);
}

// ---- the feed's argument checks ------------------------------------------------------------
void ExpectArg(int rc, const char* what, const char* needle) {
  const std::string msg = rc == DFX_OK ? "" : dfx_last_error();
  EXPECT(rc == DFX_ERR_ARG && msg.find(needle) != std::string::npos,
         "feedargs %s: status %d, message \"%s\" (want DFX_ERR_ARG naming \"%s\")", what, rc,
         msg.c_str(), needle);
}

int ModeFeedArgs(dfx_ctx* c) {
  Dev dstat(c, 32);
  const int64_t zero[4] = {0, 0, 0, 0};
  dstat.Up(zero, 32);
  const uint64_t off[2] = {0, 3}, idx[3] = {1, 2, 3};
  const float val[3] = {1.f, 2.f, 3.f}, lab[1] = {1.f};
  for (const bool libsvm : {false, true}) {
    const char* name = libsvm ? "libsvm" : "criteo";
    DeviceTextFeed feed(c, 4, 8, name);
    dfx_textfeed* f = feed.h();
    dfx_batch b;
    if (libsvm) {
      ExpectArg(dfx_textfeed_upload(f, 0, 1, 3, off, idx, nullptr, lab, nullptr),
                "libsvm upload without values", "textfeed_upload");
    } else {
      ExpectArg(dfx_textfeed_batch_end(f, 1, 3, 1, &b), "criteo batch_end valued", "Criteo feed");
      ExpectArg(dfx_textfeed_slot_batch(f, 0, 1, &b), "criteo slot_batch valued", "Criteo feed");
      ExpectArg(dfx_textfeed_upload(f, 0, 1, 3, off, idx, val, lab, nullptr),
                "criteo upload with values", "Criteo feed");
    }
    ExpectArg(dfx_textfeed_gather(f, -1, 0, nullptr, 0, 1, 0, 0), "shuffle buffer onto itself",
              "onto itself");
    ExpectArg(dfx_textfeed_gather(f, 0, 1, nullptr, 0, 1, 0, 0), "gather before batch_begin",
              "no batch begun");
    // the feed is still usable: three rows through it
    const std::string text = libsvm ? "1 3:0.5 7\n0 2:1\n1 5:2.5 6:1 9\n"
                                    : "1\t5\t\tab\n0\t\t7\n1\tx\ty\tz\n";
    Block want;
    if (libsvm)
      want = HostParse(text);
    else
      ParseCriteo(text.data(), text.data() + text.size(), true, &want);
    char* pinned = nullptr;
    DfxCheck(dfx_textfeed_text(f, 0, (int64_t)text.size(), &pinned), "dfx_textfeed_text");
    std::memcpy(pinned, text.data(), text.size());
    const int64_t blanks = std::count(text.begin(), text.end(), ' ');
    DfxCheck(dfx_textfeed_submit(f, 0, (int64_t)text.size(), 1, 3, blanks), "dfx_textfeed_submit");
    int64_t stat[4];
    const uint64_t* h_off = nullptr;
    const float* h_lab = nullptr;
    const uint8_t* h_flag = nullptr;
    DfxCheck(dfx_textfeed_wait(f, 0, stat, &h_off, &h_lab, &h_flag), "dfx_textfeed_wait");
    EXPECT(stat[0] == 3 && stat[1] == (int64_t)want.index.size() && !stat[2] && !stat[3],
           "feedargs %s: stat %lld %lld %lld %lld", name, (long long)stat[0], (long long)stat[1],
           (long long)stat[2], (long long)stat[3]);
    EXPECT((h_flag != nullptr) == libsvm, "feedargs %s: row flags handed out: %d", name,
           (int)(h_flag != nullptr));
    if (stat[0] != 3 || stat[2]) continue;
    bool valued = false;
    for (int r = 0; h_flag && r < 3; ++r) valued = valued || h_flag[r];
    EXPECT(valued == libsvm, "feedargs %s: flagged rows: %d", name, (int)valued);
    DfxCheck(dfx_textfeed_batch_begin(f), "dfx_textfeed_batch_begin");
    DfxCheck(dfx_textfeed_gather(f, 0, 1, nullptr, 0, 3, 0, libsvm ? (int64_t)h_off[3] : 0),
             "dfx_textfeed_gather");
    DfxCheck(dfx_textfeed_batch_end(f, 3, stat[1], valued ? 1 : 0, &b), "dfx_textfeed_batch_end");
    EXPECT(SameDeviceBatch(c, &dstat, want, b), "feedargs %s: the batch != the host parser's block",
           name);
    std::printf("feedargs %s: rejections and a %lld-feature chunk ok\n", name, (long long)stat[1]);
  }
  return 0;
}

int ModePlan(const std::string& path) {
  const size_t bs = 257, chunk = 64 << 10;
  size_t valued = 0, binary = 0;
  for (size_t shuffle : {(size_t)0, (size_t)3})
    for (float neg : {1.f, 0.7f})
      for (int pp = 0; pp < 2; ++pp) {
        const int part = pp, nparts = pp + 1;
        BatchReader want(path, "libsvm", part, nparts, bs, bs * shuffle, neg, 4, chunk);
        TextReader chunks(path, "libsvm", part, nparts, chunk, 4);
        std::vector<Block> seq;  // the chunks by sequence number (the last one is live)
        std::vector<std::vector<uint8_t>> seq_flag;
        Block shuf, batch;
        std::vector<uint8_t> shuf_flag;
        bool batch_valued = false;
        shuf.offset.assign(1, 0);
        BatchPlanner plan(
            bs, bs * shuffle, neg,
            [&](size_t* rows, const uint64_t** off, const float** lab) {
              if (!chunks.Next()) return false;
              seq.push_back(chunks.Value());
              seq_flag.push_back(HostFlags(seq.back()));
              *rows = seq.back().Size();
              *off = reinterpret_cast<const uint64_t*>(seq.back().offset.data());
              *lab = seq.back().label.data();
              return true;
            },
            [&](const GatherOp& op) {
              const bool from_shuf = op.src == GatherOp::kShuffle;
              const Block& src = from_shuf ? shuf : seq[op.src];
              const std::vector<uint8_t>& sf = from_shuf ? shuf_flag : seq_flag[op.src];
              Block* dst = op.to_batch ? &batch : &shuf;
              if (op.r0 == 0) {
                if (op.to_batch) {
                  batch_valued = false;
                } else {
                  shuf = Block();
                  shuf.offset.assign(1, 0);
                  shuf_flag.clear();
                }
              }
              EXPECT(dst->Size() == op.r0, "plan: r0 %zu, destination holds %zu", op.r0,
                     dst->Size());
              // the flags mirrored through the copy: chunk -> shuffle buffer -> batch
              std::vector<uint8_t> moved;
              for (size_t i = 0; i < op.n; ++i)
                moved.push_back(sf[op.rows.empty() ? op.begin + i : op.rows[i]]);
              for (uint8_t f : moved) {
                if (op.to_batch)
                  batch_valued = batch_valued || f;
                else
                  shuf_flag.push_back(f);
              }
              std::vector<size_t> rows(op.rows.begin(), op.rows.end());
              GatherRows(src, rows.empty() ? nullptr : rows.data(), op.begin, op.n, dst, 2);
            });
        seq.reserve(4096);  // chunk pointers handed to the planner stay valid
        seq_flag.reserve(4096);
        size_t n = 0;
        for (;;) {
          batch = Block();
          batch.offset.assign(1, 0);
          batch_valued = false;
          size_t rows = 0, nnz = 0;
          const bool a = want.Next(), b = plan.Next(&rows, &nnz);
          EXPECT(a == b, "plan part %d/%d shuffle %zu neg %g: batch %zu: reader %d planner %d",
                 part, nparts, shuffle, neg, n, a, b);
          if (!a || !b) break;
          EXPECT(rows == batch.Size() && nnz == batch.index.size(), "plan: counts");
          if (!batch_valued) batch.value.clear();  // no flagged row: handed out without values
          EXPECT(SameHostBlock(want.Value(), batch),
                 "plan part %d/%d shuffle %zu neg %g: batch %zu differs (reader valued %d, "
                 "mirrored flags %d)",
                 part, nparts, shuffle, neg, n, (int)!want.Value().value.empty(),
                 (int)batch_valued);
          ++n;
          (want.Value().value.empty() ? binary : valued) += 1;
          if (g_fail > 5) break;
        }
        EXPECT(n > 3, "too few batches");
        std::printf("plan part %d/%d shuffle %zu neg %g: %zu batches ok\n", part, nparts,
                    shuffle, neg, n);
      }
  EXPECT(valued > 0 && binary > 0, "%zu valued and %zu binary batches: both kinds must occur",
         valued, binary);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  const std::string a2 = argc > 2 ? argv[2] : "", a3 = argc > 3 ? argv[3] : "";
  if (mode == "plan" && argc > 2) {
    ModePlan(a2);
  } else if ((mode == "parse" && argc > 2) || mode == "fallback" || mode == "gather" ||
             mode == "feedargs" || (mode == "batches" && argc > 3)) {
    dfx_ctx* c = nullptr;
    DfxCheck(dfx_ctx_create(0, "V_dim=0,max_keys=1024", &c), "dfx_ctx_create");
    if (mode == "parse") ModeParse(c, a2);
    if (mode == "fallback") ModeFallback(c);
    if (mode == "gather") ModeGather(c);
    if (mode == "batches") ModeBatches(c, a2, a3);
    if (mode == "feedargs") ModeFeedArgs(c);
    dfx_ctx_destroy(c);
  } else {
    std::fprintf(stderr,
                 "usage: %s parse FILE | fallback | gather | batches FILE DIR | feedargs | plan FILE\n",
                 argv[0]);
    return 2;
  }
  if (g_fail) {
    std::printf("%d FAILED\n", g_fail);
    return 1;
  }
  std::printf("ALL PASSED\n");
  return 0;
}
