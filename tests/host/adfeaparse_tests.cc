// adfeaparse_tests — the device adfea path against the host reader (the yardstick is
// difacto_amd/host/reader.cc: ParseAdfea, GatherRows, BatchReader, TextReader).  Every
// comparison is exact (bytes).
//
//   GPU modes
//     parse             dfx_parse_adfea == ParseAdfea with needs_host == 0: (a) the three-row
//                       sample of reader_tests.cc; (b) nbytes 0 and 2^31, one row with no
//                       feature; (c) one line slid byte by byte over a 16-byte thread boundary
//                       and the 4 KiB tile boundary, so that a token's first digit, its ':', the
//                       gid's last digit, the blank after it and the '\n' each meet both; (d) a
//                       line over three tiles; (e) a 64-byte feature token; (f) runs of spaces
//                       and tabs before the lineid, between tokens and before '\n'; (g) the id
//                       edges (idx 0, leading zeros, 2^52 - 1, 2^52, 2^64 - 1, 2^64, 25 digits;
//                       gid 0, 4095, 4096, 2^64); (h) the labels 1 0 10 01 2 1234567890123;
//                       (i) more than 1024 tiles; (j) capacities one too small
//                       (DFX_ERR_CAPACITY, needed counts, guard words intact)
//     fallback          the forms the device must hand back (an empty line, a blank-only line,
//                       fewer than three tokens, no ':' at token >= 3, a ':' at token < 3) are
//                       flagged; CRLF, an unterminated last line, a 65-byte token and the
//                       misshapen tokens 12: :3 12:3:4 12:a -1 abc 12a, at a head place and at
//                       a feature place, are flagged or exactly ParseAdfea's output
//     batches FILE DIR  DeviceBatchReader("adfea") == BatchReader batch by batch, every batch
//                       unvalued (batch 257, 64 KB chunks, shuffle 0 / 3, neg_sampling 1 / 0.7,
//                       parts 0/1 and 1/2), whole chunks as batches, a file whose long rows make
//                       the ring entry and the shuffle buffer grow mid-run, a flagged file
//     feedargs          on an adfea feed (batch 4, shuffle buffer 8) a value array given to
//                       _upload and valued != 0 asked of _batch_end / _slot_batch are DFX_ERR_ARG
//                       with a message and queue nothing; a three-row chunk then goes text ->
//                       submit -> wait -> batch_begin -> gather -> batch_end and equals the host
//                       parser's block; a host-parsed chunk goes through _upload with value ==
//                       NULL; the Criteo and libsvm feeds behave as before
//   CPU mode (no HIP call)
//     plan FILE         BatchPlanner's plan carried out with GatherRows on binary rows of
//                       varying length == BatchReader
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

// ParseAdfea over the whole text: inside the device's domain TextReader::ParseChunk's cuts do
// not change the result (tests/test_adfea_ref.py), outside it the chunk is compared as one piece
Block HostParse(const std::string& text) {
  Block b;
  ParseAdfea(text.data(), text.data() + text.size(), &b);
  if (b.offset.empty()) b.offset.push_back(0);
  return b;
}

// short binary rows: 0-4 features, mixed blanks
std::string GenRows(int rows, unsigned seed, int max_nnz = 4) {
  std::mt19937_64 rng(seed);
  std::string out;
  char buf[64];
  for (int r = 0; r < rows; ++r) {
    const int nnz = (int)(rng() % (uint64_t)(max_nnz + 1));
    std::snprintf(buf, sizeof buf, "%d %d %d", r, nnz, (int)(rng() % 3 == 0));
    out += buf;
    for (int j = 0; j < nnz; ++j) {
      std::snprintf(buf, sizeof buf, "%s%u:%u", rng() % 8 ? " " : "\t", (unsigned)(rng() % 100000),
                    (unsigned)(rng() % 40));
      out += buf;
    }
    out += '\n';
  }
  return out;
}

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
  std::vector<float> label;
  bool guards_ok = true;
};

// dfx_parse_adfea of text with the given capacities; guard words stand before and after every
// output array
Parsed DeviceParse(dfx_ctx* c, const std::string& text, int64_t max_rows, int64_t max_nnz,
                   int misalign = 0) {
  Parsed out;
  const size_t G = kGuardWords * 8;
  Dev dtext(c, text.size() + 64), doff(c, (max_rows + 1) * 8 + 2 * G),
      didx(c, max_nnz * 8 + 2 * G), dlab(c, max_rows * 4 + 2 * G), dstat(c, 32);
  if (!text.empty()) dtext.Up(text.data(), text.size(), misalign);
  const std::vector<uint64_t> g(kGuardWords, kGuard);
  const size_t bytes[3] = {(size_t)(max_rows + 1) * 8, (size_t)max_nnz * 8, (size_t)max_rows * 4};
  Dev* const arr[3] = {&doff, &didx, &dlab};
  for (int a = 0; a < 3; ++a) {
    arr[a]->Up(g.data(), G, 0);
    arr[a]->Up(g.data(), G, G + bytes[a]);
  }
  DfxCheck(dfx_sync(c), "dfx_sync");
  char* const off = static_cast<char*>(doff.p) + G;
  char* const idx = static_cast<char*>(didx.p) + G;
  char* const lab = static_cast<char*>(dlab.p) + G;
  out.rc = dfx_parse_adfea(c, static_cast<char*>(dtext.p) + misalign, (int64_t)text.size(),
                           max_rows, max_nnz, reinterpret_cast<uint64_t*>(off),
                           reinterpret_cast<uint64_t*>(idx), reinterpret_cast<float*>(lab),
                           static_cast<int64_t*>(dstat.p));
  if (out.rc != DFX_OK) return out;
  out.rc = dfx_parse_criteo_wait(c, static_cast<int64_t*>(dstat.p), out.stat);
  for (int a = 0; a < 3; ++a) {
    std::vector<uint64_t> g1(kGuardWords), g2(kGuardWords);
    arr[a]->Down(g1.data(), G, 0);
    arr[a]->Down(g2.data(), G, G + bytes[a]);
    out.guards_ok = out.guards_ok && g1 == g && g2 == g;
  }
  if (out.rc == DFX_OK && !out.stat[2]) {
    const int64_t rows = out.stat[0], nnz = out.stat[1];
    out.offset.resize(rows + 1);
    out.index.resize(nnz);
    out.label.resize(rows);
    doff.Down(out.offset.data(), (rows + 1) * 8, G);
    if (nnz) didx.Down(out.index.data(), nnz * 8, G);
    if (rows) dlab.Down(out.label.data(), rows * 4, G);
  }
  return out;
}

// offsets, ids and labels byte for byte
bool SameBlock(const Block& want, const uint64_t* off, const uint64_t* idx, const float* lab,
               size_t rows, size_t nnz) {
  if (want.Size() != rows || want.index.size() != nnz) return false;
  for (size_t i = 0; i <= rows; ++i)
    if (want.offset[i] != off[i]) return false;
  if (nnz && std::memcmp(want.index.data(), idx, nnz * 8) != 0) return false;
  if (rows && std::memcmp(want.label.data(), lab, rows * 4) != 0) return false;
  return true;
}

bool SameParsed(const Block& want, const Parsed& got) {
  return want.value.empty() && SameBlock(want, got.offset.data(), got.index.data(),
                                         got.label.data(), got.label.size(), got.index.size());
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
    EXPECT(SameParsed(want, got), "%s: device block != ParseAdfea", name.c_str());
  }
  if (!quiet)
    std::printf("parse %s: %zu bytes, %zu rows, %zu features ok\n", name.c_str(), text.size(),
                want.Size(), want.index.size());
  return g_fail == before;
}

// `line` placed so that its byte `at` lands on text position `pos`: 10-byte filler rows, then
// up to 9 blanks in front of the line's lineid
std::string PlaceAt(const std::string& line, size_t at, size_t pos) {
  std::string out;
  if (pos < at) return line;
  size_t pad = pos - at;
  while (pad >= 10) {
    out += "3 1 0 7:2\n";
    pad -= 10;
  }
  out.append(pad, ' ');
  return out + line + "4 1 1 9:3\n";
}

const char* const kSample = "1 3 1 17:2 123456789:4095 5:1\n2 1 0 9:7\n3 0 1\n";

int ModeParse(dfx_ctx* c) {
  {  // (a) the known answer of reader_tests.cc
    const Block want = HostParse(kSample);
    const std::vector<uint64_t> ids = {(17ull << 12) | 2, (123456789ull << 12) | 4095,
                                       (5ull << 12) | 1, (9ull << 12) | 7};
    EXPECT(want.Size() == 3 && want.index == ids && want.label[0] == 1.f && want.label[1] == 0.f &&
               want.label[2] == 1.f && want.offset[1] == 3 && want.offset[2] == 4 &&
               want.offset[3] == 4,
           "(a) the host's block is not the known answer");
    CheckClean(c, "(a) the three-row sample", kSample);
    CheckClean(c, "(a) the three-row sample, unaligned text", kSample, 3);
  }
  CheckClean(c, "(b) one row with no feature", "7 0 1\n");
  {
    const Parsed got = DeviceParse(c, "", 4, 4);
    EXPECT(got.rc == DFX_OK && got.stat[0] == 0 && got.stat[1] == 0 && got.stat[2] == 0 &&
               got.stat[3] == 0 && got.guards_ok && got.offset.size() == 1 && got.offset[0] == 0,
           "(b) nbytes = 0");
    Dev d(c, 64);
    const int rc = dfx_parse_adfea(c, static_cast<char*>(d.p), 1ll << 31, 1, 1,
                                   static_cast<uint64_t*>(d.p), static_cast<uint64_t*>(d.p),
                                   static_cast<float*>(d.p), static_cast<int64_t*>(d.p));
    EXPECT(rc == DFX_ERR_ARG, "nbytes = 2^31: status %d", rc);
    std::printf("parse (b) nbytes 0 / 2^31 ok\n");
  }
  {  // (c) every part of a feature token on the thread and tile boundaries
    const std::string line = "12 2 1 345:67 8:9\n";
    const struct {
      const char* what;
      size_t at;
    } parts[] = {{"first digit", 7},    {"':'", 10},  {"gid's last digit", 12},
                 {"blank after it", 13}, {"'\\n'", 17}};
    int n = 0;
    for (size_t bound : {(size_t)16, (size_t)4096})
      for (const auto& p : parts)
        for (int d = -1; d <= 1; ++d) {
          char name[96];
          std::snprintf(name, sizeof name, "(c) %s at %zu%+d", p.what, bound - 1, d);
          CheckClean(c, name, PlaceAt(line, p.at, bound - 1 + d), 0, true);
          ++n;
        }
    std::printf("parse (c) %d boundary placements ok\n", n);
  }
  {  // (d) a line over three tiles: the tiles between have no newline
    std::string t = "1 1 0 2:3\n2 1500 1";
    char buf[32];
    for (int j = 0; j < 1500; ++j) {
      std::snprintf(buf, sizeof buf, " %d:%d", 100000 + j, j % 4096);
      t += buf;
    }
    t += "\n3 1 0 5:1\n";
    EXPECT(t.size() > 3 * 4096, "(d) too short");
    CheckClean(c, "(d) a line over three tiles", t);
  }
  {  // (e) the token cap: 64 bytes parse
    const std::string t64 = std::string(40, '0') + "1234567890123456789:" + "0042";
    EXPECT(t64.size() == 64, "(e) token length %zu", t64.size());
    CheckClean(c, "(e) a 64-byte feature token", "1 2 1 5:2 " + t64 + " 3:1\n2 1 0 1:1\n");
  }
  CheckClean(c, "(f) runs of blanks and tabs",
             "1 2 1 2:3  4:5\n  2 1 0 1:2\n\t3\t\t1 \t 1   3:4\t\n \t \t 4     0     0     \n"
             "5 0 1 \n6\t0\t0\t\n7 1 1 5:6\t\t\t\t\t\n");
  CheckClean(c, "(g) the id edges",
             "1 7 1 0:0 000017:0004095 4503599627370495:4095 4503599627370496:4096\n"
             "2 4 0 18446744073709551615:1 18446744073709551616:18446744073709551616 "
             "1234567890123456789012345:7 9:0\n");
  {
    const std::string t = "1 0 1\n2 0 0\n3 0 10\n4 0 01\n5 0 2\n6 0 1234567890123\n";
    const Block want = HostParse(t);
    const std::vector<float> labels = {1.f, 0.f, 1.f, 0.f, 0.f, 1.f};
    EXPECT(want.label == labels, "(h) the host's labels are not the reference's rule");
    CheckClean(c, "(h) labels", t);
  }
  {  // (i) more tiles than one pass of k_scan_totals covers (1024 tiles of 4 KiB)
    const std::string t = GenRows(190000, 5);
    EXPECT(t.size() > 1030u * 4096u, "(i) only %zu bytes", t.size());
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
  return 0;
}

int ModeFallback(dfx_ctx* c) {
  const std::string body = GenRows(50, 4);
  std::string crlf;
  for (char ch : body) {
    if (ch == '\n') crlf += '\r';
    crlf += ch;
  }
  // must: the device has to flag the form (rows = newlines or the place formula is false)
  struct Case {
    std::string name, text;
    int must;
  };
  std::vector<Case> cases = {
      {"empty line", body.substr(0, body.find('\n') + 1) + "\n" + body, 1},
      {"leading empty line", "\n" + body, 1},
      {"blank-only line", body + " \t \n" + body, 1},
      {"two tokens", body + "7 1\n" + body, 1},
      {"one token", body + "7\n" + body, 1},
      {"no ':' at token 3", body + "7 1 1 5\n" + body, 1},
      {"no ':' at token 4", body + "7 2 1 5:1 6\n" + body, 1},
      {"':' at token 0", body + "5:1 6:2\n" + body, 1},
      {"':' at token 1", body + "7 5:1 1\n" + body, 1},
      {"':' at token 2 (a continued row)", body + "7 1 5:1 6:2\n" + body, 1},
      {"CRLF", crlf, 0},
      {"unterminated last line", body.substr(0, body.size() - 1), 0},
      {"a 65-byte token", body + "7 1 1 " + std::string(61, '0') + "5:12\n" + body, 0},
  };
  for (const char* tok : {"12:", ":3", "12:3:4", "12:a", "-1", "abc", "12a"}) {
    cases.push_back({std::string("\"") + tok + "\" as a feature",
                     body + "7 2 1 " + tok + " 6:2\n" + body, 0});
    cases.push_back({std::string("\"") + tok + "\" as the count",
                     body + "7 " + tok + " 1 6:2\n" + body, 0});
  }
  for (const Case& cs : cases) {
    int64_t lines = 1, colons = 1;
    for (char ch : cs.text) {
      lines += ch == '\n';
      colons += ch == ':';
    }
    const Parsed got = DeviceParse(c, cs.text, lines, colons);
    EXPECT(got.rc == DFX_OK && got.guards_ok, "%s: status %d guards %d", cs.name.c_str(), got.rc,
           (int)got.guards_ok);
    if (got.rc != DFX_OK) continue;
    if (cs.must) {
      EXPECT(got.stat[2] == 1, "%s: not handed back", cs.name.c_str());
    } else if (!got.stat[2]) {
      EXPECT(SameParsed(HostParse(cs.text), got), "%s: not flagged and != ParseAdfea",
             cs.name.c_str());
    }
    std::printf("fallback %s: %s\n", cs.name.c_str(), got.stat[2] ? "needs_host" : "equal");
  }
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
  if (b.value && std::memcmp(want.value.data(), val.data(), b.nnz * 4) != 0) return false;
  return SameBlock(want, off.data(), idx.data(), lab.data(), b.size, b.nnz);
}

struct Counts {
  size_t batches = 0, fallback = 0;
};

Counts CompareReaders(dfx_ctx* c, Dev* dstat, DeviceTextFeed* feed, const std::string& path,
                      int part, int nparts, size_t bs, size_t shuffle, float neg, size_t chunk) {
  BatchReader host(path, "adfea", part, nparts, bs, bs * shuffle, neg, 4, chunk);
  DeviceBatchReader dev(feed, path, "adfea", part, nparts, bs, bs * shuffle, neg, 4, chunk);
  Counts n;
  for (;;) {
    const bool a = host.Next(), b = dev.Next();
    EXPECT(a == b, "part %d/%d shuffle %zu neg %g: batch %zu: host %d device %d", part, nparts,
           shuffle, neg, n.batches, a, b);
    if (!a || !b) break;
    EXPECT(host.Value().value.empty(), "the host reader's adfea batch has values");
    EXPECT(SameDeviceBatch(c, dstat, host.Value(), dev.Value()),
           "part %d/%d shuffle %zu neg %g: batch %zu differs", part, nparts, shuffle, neg,
           n.batches);
    dev.Consumed();
    ++n.batches;
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
  DeviceTextFeed feed(c, bs, bs * 3, "adfea");
  for (size_t shuffle : {(size_t)0, (size_t)3})
    for (float neg : {1.f, 0.7f})
      for (int pp = 0; pp < 2; ++pp) {
        const Counts n =
            CompareReaders(c, &dstat, &feed, path, pp, pp + 1, bs, shuffle, neg, 64 << 10);
        std::printf("batches part %d/%d shuffle %zu neg %g: %zu batches (unvalued) ok\n", pp,
                    pp + 1, shuffle, neg, n.batches);
        EXPECT(n.batches > 3 && n.fallback == 0, "%zu batches, %zu fallback chunks", n.batches,
               n.fallback);
      }
  {  // every chunk one batch (validation, prediction)
    TextReader host(path, "adfea", 0, 1, 64 << 10, 4);
    DeviceBatchReader dev(&feed, path, "adfea", 0, 1, 0, 0, 1.f, 4, 64 << 10);
    size_t n = 0;
    for (;;) {
      bool a;
      do {
        a = host.Next();
      } while (a && host.Value().Size() == 0);
      const bool b = dev.Next();
      EXPECT(a == b, "whole chunks: chunk %zu: host %d device %d", n, a, b);
      if (!a || !b) break;
      const Block& want = host.Value();
      EXPECT(SameDeviceBatch(c, &dstat, want, dev.Value()), "whole chunk %zu differs", n);
      EXPECT(std::memcmp(dev.HostLabels(), want.label.data(), want.Size() * 4) == 0,
             "whole chunk %zu: host labels differ", n);
      dev.Consumed();
      ++n;
    }
    EXPECT(dev.FallbackChunks() == 0, "whole chunks: %zu parsed by the host",
           dev.FallbackChunks());
    std::printf("batches whole chunks: %zu ok\n", n);
    EXPECT(n > 3, "whole chunks: %zu", n);
  }
  {  // rows of ~50,000 features among short ones: the ring entry and the shuffle buffer grow
    const std::string grow = dir + "/grow.adfea";
    std::string out;
    char buf[48];
    for (int r = 0; r < 1400; ++r) {
      if (r == 130 || r == 400 || r == 610) {
        std::snprintf(buf, sizeof buf, "%d %d 1", r, 50000 + r);
        out += buf;
        for (int j = 0; j < 50000 + r; ++j) {
          std::snprintf(buf, sizeof buf, " %d:%d", j * 3 + r, (j * 7 + r) % 4096);
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
  {  // a file the device hands back: lines with a bare feature token, CRLF line ends.  Every
     // line keeps ParseAdfea's counter at 0 at its end, so the host's result is cut-independent
    const std::string bad = dir + "/needs_host.adfea";
    const std::string text = GenRows(9000, 9);
    std::string out;
    for (size_t i = 0, line = 0; i < text.size(); ++i) {
      if (text[i] == '\n') {
        ++line;
        if (line % 2000 == 0) out += " 77:x";
        if (line % 3100 == 0) out += '\r';
      }
      out += text[i];
    }
    std::ofstream(bad, std::ios::binary) << out;
    const Counts n = CompareReaders(c, &dstat, &feed, bad, 0, 1, bs, 3, 0.7f, 16 << 10);
    EXPECT(n.batches > 0 && n.fallback >= 3 && n.fallback <= 6,
           "needs_host file: %zu batches, %zu fallback chunks", n.batches, n.fallback);
    std::printf("batches needs_host file: %zu batches, %zu chunks parsed by the host ok\n",
                n.batches, n.fallback);
  }
  {  // one line with more tokens at feature places than the chunk has ':' bytes, the reader's
     // bound for its features: the chunk needs more than its capacity and is handed back too
    const std::string over = dir + "/over_bound.adfea";
    const std::string text = GenRows(300, 10);
    const size_t at = text.find('\n', text.size() / 2);
    std::ofstream(over, std::ios::binary)
        << text.substr(0, at) + " 5 6 7 8 9 10" + text.substr(at);
    const Counts n = CompareReaders(c, &dstat, &feed, over, 0, 1, bs, 0, 1.f, 64 << 10);
    EXPECT(n.batches > 0 && n.fallback == 1, "over_bound file: %zu batches, %zu fallback chunks",
           n.batches, n.fallback);
    std::printf("batches over_bound file: %zu batches, %zu chunk parsed by the host ok\n",
                n.batches, n.fallback);
  }
  return 0;
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
  for (const char* name : {"criteo", "libsvm", "adfea"}) {
    const std::string fmt = name;
    const bool libsvm = fmt == "libsvm", adfea = fmt == "adfea";
    DeviceTextFeed feed(c, 4, 8, name);
    dfx_textfeed* f = feed.h();
    EXPECT(feed.format() == (adfea ? DFX_TEXT_ADFEA : libsvm ? DFX_TEXT_LIBSVM : DFX_TEXT_CRITEO),
           "feedargs %s: format %d", name, feed.format());
    dfx_batch b;
    if (libsvm) {
      ExpectArg(dfx_textfeed_upload(f, 0, 1, 3, off, idx, nullptr, lab, nullptr),
                "libsvm upload without values", "textfeed_upload");
    } else {
      const char* needle = adfea ? "adfea feed" : "Criteo feed";
      ExpectArg(dfx_textfeed_batch_end(f, 1, 3, 1, &b), "batch_end valued", needle);
      ExpectArg(dfx_textfeed_slot_batch(f, 0, 1, &b), "slot_batch valued", needle);
      ExpectArg(dfx_textfeed_upload(f, 0, 1, 3, off, idx, val, lab, nullptr),
                "upload with values", needle);
    }
    ExpectArg(dfx_textfeed_gather(f, -1, 0, nullptr, 0, 1, 0, 0), "shuffle buffer onto itself",
              "onto itself");
    ExpectArg(dfx_textfeed_gather(f, 0, 1, nullptr, 0, 1, 0, 0), "gather before batch_begin",
              "no batch begun");
    // the rejected calls queued nothing and the feed is still usable: three rows through it
    const std::string text = libsvm  ? "1 3:0.5 7\n0 2:1\n1 5:2.5 6:1 9\n"
                             : adfea ? kSample
                                     : "1\t5\t\tab\n0\t\t7\n1\tx\ty\tz\n";
    Block want;
    if (libsvm)
      ParseLibSVM(text.data(), text.data() + text.size(), &want);
    else if (adfea)
      want = HostParse(text);
    else
      ParseCriteo(text.data(), text.data() + text.size(), true, &want);
    char* pinned = nullptr;
    DfxCheck(dfx_textfeed_text(f, 0, (int64_t)text.size(), &pinned), "dfx_textfeed_text");
    std::memcpy(pinned, text.data(), text.size());
    const int64_t bound = adfea ? std::count(text.begin(), text.end(), ':')
                                : std::count(text.begin(), text.end(), ' ');
    DfxCheck(dfx_textfeed_submit(f, 0, (int64_t)text.size(), 1, 3, bound), "dfx_textfeed_submit");
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
    if (!valued) want.value.clear();
    DfxCheck(dfx_textfeed_batch_begin(f), "dfx_textfeed_batch_begin");
    const int64_t gather_nnz = fmt == "criteo" ? 0 : (int64_t)h_off[3];
    DfxCheck(dfx_textfeed_gather(f, 0, 1, nullptr, 0, 3, 0, gather_nnz), "dfx_textfeed_gather");
    DfxCheck(dfx_textfeed_batch_end(f, 3, stat[1], valued ? 1 : 0, &b), "dfx_textfeed_batch_end");
    EXPECT(SameDeviceBatch(c, &dstat, want, b), "feedargs %s: the batch != the host parser's block",
           name);
    DfxCheck(dfx_textfeed_consumed(f), "dfx_textfeed_consumed");
    if (adfea) {  // a host-parsed chunk: _upload with value == NULL, then the slot as a batch
      const uint8_t* up_flag = reinterpret_cast<const uint8_t*>(&b);
      DfxCheck(dfx_textfeed_upload(f, 1, (int64_t)want.Size(), (int64_t)want.index.size(),
                                   reinterpret_cast<const uint64_t*>(want.offset.data()),
                                   want.index.data(), nullptr, want.label.data(), &up_flag),
               "dfx_textfeed_upload");
      EXPECT(up_flag == nullptr, "feedargs adfea: _upload handed out row flags");
      DfxCheck(dfx_textfeed_slot_batch(f, 1, 0, &b), "dfx_textfeed_slot_batch");
      EXPECT(SameDeviceBatch(c, &dstat, want, b), "feedargs adfea: the uploaded chunk differs");
      DfxCheck(dfx_textfeed_slot_consumed(f, 1), "dfx_textfeed_slot_consumed");
    }
    std::printf("feedargs %s: rejections and a %lld-feature chunk ok\n", name, (long long)stat[1]);
  }
  return 0;
}

// ---- the CPU mode ------------------------------------------------------------------------
bool SameHostBlock(const Block& a, const Block& b) {
  return a.Size() == b.Size() && a.offset == b.offset && a.index == b.index &&
         a.label.size() == b.label.size() && a.value.size() == b.value.size() &&
         (a.label.empty() ||
          std::memcmp(a.label.data(), b.label.data(), a.label.size() * 4) == 0);
}

int ModePlan(const std::string& path) {
  const size_t bs = 257, chunk = 64 << 10;
  for (size_t shuffle : {(size_t)0, (size_t)3})
    for (float neg : {1.f, 0.7f})
      for (int pp = 0; pp < 2; ++pp) {
        const int part = pp, nparts = pp + 1;
        BatchReader want(path, "adfea", part, nparts, bs, bs * shuffle, neg, 4, chunk);
        TextReader chunks(path, "adfea", part, nparts, chunk, 4);
        std::vector<Block> seq;  // the chunks by sequence number (the last one is live)
        Block shuf, batch;
        shuf.offset.assign(1, 0);
        size_t min_len = ~(size_t)0, max_len = 0;
        BatchPlanner plan(
            bs, bs * shuffle, neg,
            [&](size_t* rows, const uint64_t** off, const float** lab) {
              if (!chunks.Next()) return false;
              seq.push_back(chunks.Value());
              const Block& b = seq.back();
              EXPECT(b.value.empty(), "plan: an adfea chunk with values");
              for (size_t r = 0; r < b.Size(); ++r) {
                min_len = std::min<size_t>(min_len, b.offset[r + 1] - b.offset[r]);
                max_len = std::max<size_t>(max_len, b.offset[r + 1] - b.offset[r]);
              }
              *rows = b.Size();
              *off = reinterpret_cast<const uint64_t*>(b.offset.data());
              *lab = b.label.data();
              return true;
            },
            [&](const GatherOp& op) {
              const bool from_shuf = op.src == GatherOp::kShuffle;
              const Block& src = from_shuf ? shuf : seq[op.src];
              Block* dst = op.to_batch ? &batch : &shuf;
              if (op.r0 == 0 && !op.to_batch) {
                shuf = Block();
                shuf.offset.assign(1, 0);
              }
              EXPECT(dst->Size() == op.r0, "plan: r0 %zu, destination holds %zu", op.r0,
                     dst->Size());
              std::vector<size_t> rows(op.rows.begin(), op.rows.end());
              GatherRows(src, rows.empty() ? nullptr : rows.data(), op.begin, op.n, dst, 2);
            });
        seq.reserve(4096);  // chunk pointers handed to the planner stay valid
        size_t n = 0;
        for (;;) {
          batch = Block();
          batch.offset.assign(1, 0);
          size_t rows = 0, nnz = 0;
          const bool a = want.Next(), b = plan.Next(&rows, &nnz);
          EXPECT(a == b, "plan part %d/%d shuffle %zu neg %g: batch %zu: reader %d planner %d",
                 part, nparts, shuffle, neg, n, a, b);
          if (!a || !b) break;
          EXPECT(rows == batch.Size() && nnz == batch.index.size(), "plan: counts");
          batch.value.clear();  // binary rows: handed out without values
          EXPECT(SameHostBlock(want.Value(), batch),
                 "plan part %d/%d shuffle %zu neg %g: batch %zu differs", part, nparts, shuffle,
                 neg, n);
          ++n;
          if (g_fail > 5) break;
        }
        EXPECT(n > 3, "too few batches");
        EXPECT(min_len < max_len, "plan: the rows all have %zu features", max_len);
        std::printf("plan part %d/%d shuffle %zu neg %g: %zu batches ok\n", part, nparts,
                    shuffle, neg, n);
      }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  const std::string a2 = argc > 2 ? argv[2] : "", a3 = argc > 3 ? argv[3] : "";
  if (mode == "plan" && argc > 2) {
    ModePlan(a2);
  } else if (mode == "parse" || mode == "fallback" || mode == "feedargs" ||
             (mode == "batches" && argc > 3)) {
    dfx_ctx* c = nullptr;
    DfxCheck(dfx_ctx_create(0, "V_dim=0,max_keys=1024", &c), "dfx_ctx_create");
    if (mode == "parse") ModeParse(c);
    if (mode == "fallback") ModeFallback(c);
    if (mode == "batches") ModeBatches(c, a2, a3);
    if (mode == "feedargs") ModeFeedArgs(c);
    dfx_ctx_destroy(c);
  } else {
    std::fprintf(stderr, "usage: %s parse | fallback | batches FILE DIR | feedargs | plan FILE\n",
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
