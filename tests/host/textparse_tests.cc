// textparse_tests — the device text path against the host reader (the yardstick is
// difacto_amd/host/reader.cc: ParseCriteo, GatherRows, BatchReader, TextReader).
//
//   GPU modes
//     parse             dfx_parse_criteo == ParseCriteo, exactly, for both is_train values, with
//                       needs_host == 0: generated rows, a cell-length sweep over every
//                       CityHash64 branch, 0..39 / 45 columns and empty rows (label-only lines
//                       included), one row, 70,000 rows, an unaligned text pointer; capacities
//                       one too small (DFX_ERR_CAPACITY, guard words intact); nbytes 0 and 2^31
//     fallback          CRLF, blank lines, labels 1.5 / abc / empty / +1, an unterminated last
//                       line: flagged (needs_host) or exactly ParseCriteo's output
//     gather            dfx_gather_rows == GatherRows: range, permuted list, list with gaps,
//                       n = 0, appending at r0 > 0, zero-length source rows
//     batches FILE DIR  DeviceBatchReader == BatchReader batch by batch (batch 257, 64 KB
//                       chunks, shuffle 0 / 3, neg_sampling 1 / 0.7, parts 0/1 and 1/2), whole
//                       chunks as batches, and a flagged file through the host fallback
//   CPU modes (no HIP call)
//     plan FILE         BatchPlanner's plan carried out with GatherRows == BatchReader
//     cuts FILE DIR     TextReader::NextRaw chunks parsed by ParseCriteo == TextReader::Next
//     hashcells         "cell<TAB>CityHash64" of the sweep's cells (tests/golden pins them)
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

// ---- chunk generators -------------------------------------------------------------------
// rows in tools/gen_criteo.cc's shape: a 0/1 label, 13 integer and 26 8-hex-digit columns, 5%
// of the cells empty
std::string GenRows(int rows, unsigned seed) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::string out;
  char buf[32];
  for (int r = 0; r < rows; ++r) {
    out += U(rng) < 0.25 ? '1' : '0';
    for (int j = 0; j < 39; ++j) {
      out += '\t';
      if (U(rng) < 0.05) continue;
      if (j < 13) {
        std::snprintf(buf, sizeof(buf), "%d", (int)(U(rng) * 1000));
      } else {
        std::snprintf(buf, sizeof(buf), "%08x", (unsigned)(rng() & 0xffffffffu));
      }
      out += buf;
    }
    out += '\n';
  }
  return out;
}

const int kSweepLens[] = {1, 3, 4, 7, 8, 16, 17, 32, 33, 64, 65, 127, 128, 129, 200};

std::string SweepCell(int len, int col, int row) {
  static const char abc[] = "abcdefghijklmnopqrstuvwxyz0123456789";
  std::string c(len, 'a');
  for (int k = 0; k < len; ++k) c[k] = abc[(k * 7 + len * 13 + col * 5 + row * 3 + k * k) % 36];
  return c;
}

// rows whose 39 cells all have one length, for every length of the sweep
std::string GenSweep() {
  std::string out;
  for (int len : kSweepLens)
    for (int r = 0; r < 2; ++r) {
      out += r ? '1' : '0';
      for (int j = 0; j < 39; ++j) out += '\t' + SweepCell(len, j, r);
      out += '\n';
    }
  return out;
}

// k feature columns for k = 0..39 (k = 0: a line holding only its label, which takes the next
// line's cells in a training file), 45 columns, 39 empty cells, runs of label-only lines
std::string GenColumns() {
  std::string out;
  char buf[32];
  for (int k = 0; k <= 39; ++k) {
    out += k % 3 ? "1" : "0";
    for (int j = 0; j < k; ++j) {
      std::snprintf(buf, sizeof(buf), "\t%x", 1000 * k + j);
      out += buf;
    }
    out += '\n';
  }
  out += "1";
  for (int j = 0; j < 45; ++j) {
    std::snprintf(buf, sizeof(buf), "\tw%d", j);
    out += buf;
  }
  out += "\n0";
  out.append(39, '\t');
  out += "\n1\n0\n1\n7\tx\ty\n0\n";  // label-only lines: three in a row, then one at the end
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

// dfx_parse_criteo of text with the given capacities; guard words follow every output array
Parsed DeviceParse(dfx_ctx* c, const std::string& text, int is_train, int64_t max_rows,
                   int64_t max_nnz, int misalign = 0) {
  Parsed out;
  Dev dtext(c, text.size() + 64), doff(c, (max_rows + 1 + kGuardWords) * 8),
      didx(c, (max_nnz + kGuardWords) * 8), dlab(c, max_rows * 4 + kGuardWords * 8), dstat(c, 32);
  if (!text.empty()) dtext.Up(text.data(), text.size(), misalign);
  std::vector<uint64_t> g(kGuardWords, kGuard);
  doff.Up(g.data(), kGuardWords * 8, (max_rows + 1) * 8);
  didx.Up(g.data(), kGuardWords * 8, max_nnz * 8);
  dlab.Up(g.data(), kGuardWords * 8, max_rows * 4);
  DfxCheck(dfx_sync(c), "dfx_sync");
  out.rc = dfx_parse_criteo(c, static_cast<char*>(dtext.p) + misalign, (int64_t)text.size(),
                            is_train, max_rows, max_nnz, static_cast<uint64_t*>(doff.p),
                            static_cast<uint64_t*>(didx.p), static_cast<float*>(dlab.p),
                            static_cast<int64_t*>(dstat.p));
  if (out.rc != DFX_OK) return out;
  out.rc = dfx_parse_criteo_wait(c, static_cast<int64_t*>(dstat.p), out.stat);
  std::vector<uint64_t> g1(kGuardWords), g2(kGuardWords), g3(kGuardWords);
  doff.Down(g1.data(), kGuardWords * 8, (max_rows + 1) * 8);
  didx.Down(g2.data(), kGuardWords * 8, max_nnz * 8);
  dlab.Down(g3.data(), kGuardWords * 8, max_rows * 4);
  out.guards_ok = g1 == g && g2 == g && g3 == g;
  if (out.rc == DFX_OK && !out.stat[2]) {
    const int64_t rows = out.stat[0], nnz = out.stat[1];
    out.offset.resize(rows + 1);
    out.index.resize(nnz);
    out.label.resize(rows);
    doff.Down(out.offset.data(), (rows + 1) * 8);
    if (nnz) didx.Down(out.index.data(), nnz * 8);
    if (rows) dlab.Down(out.label.data(), rows * 4);
  }
  return out;
}

bool SameBlock(const Block& want, const uint64_t* off, const uint64_t* idx, const float* lab,
               size_t rows, size_t nnz) {
  if (want.Size() != rows || want.index.size() != nnz) return false;
  for (size_t i = 0; i <= rows; ++i)
    if (want.offset[i] != off[i]) return false;
  if (nnz && std::memcmp(want.index.data(), idx, nnz * 8) != 0) return false;
  if (rows && std::memcmp(want.label.data(), lab, rows * 4) != 0) return false;  // bit-equal
  return true;
}

Block HostParse(const std::string& text, bool is_train) {
  Block b;
  ParseCriteo(text.data(), text.data() + text.size(), is_train, &b);
  return b;
}

// exact capacities: the device must match the host and stay inside them
void CheckClean(dfx_ctx* c, const char* name, const std::string& text, int misalign = 0) {
  for (int is_train = 1; is_train >= 0; --is_train) {
    const Block want = HostParse(text, is_train != 0);
    const Parsed got = DeviceParse(c, text, is_train, (int64_t)want.Size(),
                                   (int64_t)want.index.size(), misalign);
    EXPECT(got.rc == DFX_OK, "%s is_train=%d: status %d (%s)", name, is_train, got.rc,
           dfx_last_error());
    EXPECT(got.guards_ok, "%s is_train=%d: guard words overwritten", name, is_train);
    EXPECT(got.stat[2] == 0, "%s is_train=%d: needs_host raised", name, is_train);
    EXPECT(got.stat[3] == 0, "%s is_train=%d: overflow raised", name, is_train);
    if (got.rc != DFX_OK || got.stat[2]) continue;
    EXPECT((size_t)got.stat[0] == want.Size() && (size_t)got.stat[1] == want.index.size(),
           "%s is_train=%d: %lld rows %lld ids, host %zu %zu", name, is_train,
           (long long)got.stat[0], (long long)got.stat[1], want.Size(), want.index.size());
    EXPECT(SameBlock(want, got.offset.data(), got.index.data(), got.label.data(),
                     got.label.size(), got.index.size()),
           "%s is_train=%d: device block != ParseCriteo", name, is_train);
  }
  std::printf("parse %s: %zu bytes ok\n", name, text.size());
}

int ModeParse(dfx_ctx* c) {
  const std::string a = GenRows(2000, 1);
  CheckClean(c, "(a) generated rows", a);
  CheckClean(c, "(a) generated rows, unaligned text", a, 3);
  CheckClean(c, "(b) cell-length sweep", GenSweep());
  CheckClean(c, "(c) 0..39 / 45 columns, empty cells, label-only lines", GenColumns());
  CheckClean(c, "(d) one row", GenRows(1, 2));
  CheckClean(c, "(e) 70,000 rows", GenRows(70000, 3));
  // (f) capacities one too small
  for (int is_train = 1; is_train >= 0; --is_train) {
    const Block want = HostParse(a, is_train != 0);
    const int64_t rows = want.Size(), nnz = want.index.size();
    for (int which = 0; which < 2; ++which) {
      const Parsed got = DeviceParse(c, a, is_train, rows - (which == 0), nnz - (which == 1));
      EXPECT(got.rc == DFX_ERR_CAPACITY, "(f) is_train=%d %s too small: status %d", is_train,
             which ? "max_nnz" : "max_rows", got.rc);
      EXPECT(got.stat[3] == 1 && got.stat[0] >= rows && got.stat[1] >= nnz,
             "(f) needed counts %lld %lld, host %lld %lld", (long long)got.stat[0],
             (long long)got.stat[1], (long long)rows, (long long)nnz);
      if (is_train || which)  // every line within the per-line arrays: the counts are exact
        EXPECT(got.stat[0] == rows && got.stat[1] == nnz, "(f) needed counts not exact");
      EXPECT(got.guards_ok, "(f) guard words overwritten");
    }
  }
  std::printf("parse (f) capacity ok\n");
  // (g) nothing to parse; positions are 32-bit
  for (int is_train = 1; is_train >= 0; --is_train) {
    const Parsed got = DeviceParse(c, "", is_train, 4, 4);
    EXPECT(got.rc == DFX_OK && got.stat[0] == 0 && got.stat[1] == 0 && got.stat[2] == 0 &&
               got.stat[3] == 0 && got.guards_ok && got.offset.size() == 1 && got.offset[0] == 0,
           "(g) nbytes = 0");
  }
  {
    Dev d(c, 64);
    const int rc = dfx_parse_criteo(c, static_cast<char*>(d.p), 1ll << 31, 1, 1, 1,
                                    static_cast<uint64_t*>(d.p), static_cast<uint64_t*>(d.p),
                                    static_cast<float*>(d.p), static_cast<int64_t*>(d.p));
    EXPECT(rc == DFX_ERR_ARG, "nbytes = 2^31: status %d", rc);
  }
  std::printf("parse (g) ok\n");
  return 0;
}

int ModeFallback(dfx_ctx* c) {
  const std::string body = GenRows(50, 4);
  std::string crlf;
  for (char ch : body) {
    if (ch == '\n') crlf += '\r';
    crlf += ch;
  }
  const std::string row = GenRows(1, 5).substr(1);  // "\t..\n": a row without its label
  struct Case {
    const char* name;
    std::string text;
    int must_be_clean;  // 1: inside the fast grammar, the device may not hand it back
  } cases[] = {
      {"CRLF", crlf, 0},
      {"blank lines", body.substr(0, 600) + "\n\n" + body.substr(600) + "\n", 0},
      {"leading blank line", "\n" + body, 0},
      {"label 1.5", body + "1.5" + row + body, 0},
      {"label abc", body + "abc" + row, 0},
      {"empty label", row + body, 0},
      {"label +1", body + "+1" + row + "-0" + row + "007" + row, 1},
      {"unterminated last line", body.substr(0, body.size() - 1), 0},
  };
  for (const Case& cs : cases) {
    for (int is_train = 1; is_train >= 0; --is_train) {
      const Block want = HostParse(cs.text, is_train != 0);
      int64_t lines = 1;
      for (char ch : cs.text) lines += ch == '\n';
      const Parsed got = DeviceParse(c, cs.text, is_train, lines, 39 * lines);
      EXPECT(got.rc == DFX_OK && got.guards_ok, "%s is_train=%d: status %d", cs.name, is_train,
             got.rc);
      if (got.rc != DFX_OK) continue;
      if (cs.must_be_clean) EXPECT(got.stat[2] == 0, "%s: needs_host raised", cs.name);
      if (!got.stat[2])
        EXPECT(SameBlock(want, got.offset.data(), got.index.data(), got.label.data(),
                         got.label.size(), got.index.size()),
               "%s is_train=%d: not flagged and != ParseCriteo", cs.name, is_train);
      std::printf("fallback %s is_train=%d: %s\n", cs.name, is_train,
                  got.stat[2] ? "needs_host" : "equal");
    }
  }
  return 0;
}

// ---- gather ------------------------------------------------------------------------------
int ModeGather(dfx_ctx* c) {
  const Block src = HostParse(GenRows(500, 6) + GenColumns() + GenRows(300, 7), true);
  const size_t R = src.Size(), N = src.index.size();
  Dev soff(c, (R + 1) * 8), sidx(c, N * 8), slab(c, R * 4);
  soff.Up(src.offset.data(), (R + 1) * 8);
  sidx.Up(src.index.data(), N * 8);
  slab.Up(src.label.data(), R * 4);
  const size_t cap_rows = 2 * R, cap_nnz = 2 * N;
  Dev doff(c, (cap_rows + 1) * 8), didx(c, cap_nnz * 8), dlab(c, cap_rows * 4), drows(c, R * 4);
  Block want;
  std::mt19937 rng(3);
  auto step = [&](const char* name, const std::vector<size_t>* rows, size_t begin, size_t n) {
    std::vector<uint32_t> r32;
    if (rows) {
      for (size_t r : *rows) r32.push_back((uint32_t)r);
      if (n) drows.Up(r32.data(), n * 4);
    }
    const size_t r0 = want.Size();
    const int rc = dfx_gather_rows(c, static_cast<uint64_t*>(soff.p), static_cast<uint64_t*>(sidx.p),
                                   static_cast<float*>(slab.p),
                                   rows ? static_cast<uint32_t*>(drows.p) : nullptr,
                                   (int64_t)begin, (int64_t)n, static_cast<uint64_t*>(doff.p),
                                   static_cast<uint64_t*>(didx.p), static_cast<float*>(dlab.p),
                                   (int64_t)r0);
    EXPECT(rc == DFX_OK, "gather %s: status %d (%s)", name, rc, dfx_last_error());
    GatherRows(src, rows ? rows->data() : nullptr, begin, n, &want, 2);
    const size_t rows_now = want.Size(), nnz_now = want.index.size();
    if (rows_now == 0) return;
    std::vector<uint64_t> off(rows_now + 1), idx(nnz_now);
    std::vector<float> lab(rows_now);
    doff.Down(off.data(), (rows_now + 1) * 8);
    if (nnz_now) didx.Down(idx.data(), nnz_now * 8);
    dlab.Down(lab.data(), rows_now * 4);
    EXPECT(SameBlock(want, off.data(), idx.data(), lab.data(), rows_now, nnz_now),
           "gather %s: device block != GatherRows", name);
    std::printf("gather %s: %zu rows %zu ids ok\n", name, rows_now, nnz_now);
  };
  step("n = 0 into an empty destination", nullptr, 0, 0);
  step("range at r0 = 0", nullptr, 490, 80);  // spans the zero-length rows
  std::vector<size_t> perm(R);
  for (size_t i = 0; i < R; ++i) perm[i] = i;
  std::shuffle(perm.begin(), perm.end(), rng);
  perm.resize(300);
  step("permuted list at r0 > 0", &perm, 0, perm.size());
  std::vector<size_t> gaps;
  for (size_t i = 2; i < R; i += 7) gaps.push_back(i);
  step("list with gaps", &gaps, 0, gaps.size());
  step("n = 0", &gaps, 0, 0);
  step("one row", nullptr, R - 1, 1);
  step("range at r0 > 0", nullptr, 0, 257);
  return 0;
}

// ---- batches -----------------------------------------------------------------------------
void JoinInput(dfx_ctx* c, Dev* dstat) {
  int64_t stat[4];
  DfxCheck(dfx_parse_criteo_wait(c, static_cast<int64_t*>(dstat->p), stat), "join input stream");
}

bool SameDeviceBatch(dfx_ctx* c, Dev* dstat, const Block& want, const dfx_batch& b) {
  JoinInput(c, dstat);
  if ((size_t)b.size != want.Size() || (size_t)b.nnz != want.index.size()) return false;
  std::vector<uint64_t> off(b.size + 1), idx(b.nnz);
  std::vector<float> lab(b.size);
  DfxCheck(dfx_memcpy(c, off.data(), b.offset, (b.size + 1) * 8, 1), "download");
  if (b.nnz) DfxCheck(dfx_memcpy(c, idx.data(), b.index, b.nnz * 8, 1), "download");
  DfxCheck(dfx_memcpy(c, lab.data(), b.label, b.size * 4, 1), "download");
  return SameBlock(want, off.data(), idx.data(), lab.data(), b.size, b.nnz);
}

size_t CompareReaders(dfx_ctx* c, Dev* dstat, DeviceTextFeed* feed, const std::string& path,
                      int part, int nparts, size_t bs, size_t shuffle, float neg, size_t chunk,
                      size_t* fallback) {
  BatchReader host(path, "criteo", part, nparts, bs, bs * shuffle, neg, 4, chunk);
  DeviceBatchReader dev(feed, path, "criteo", part, nparts, bs, bs * shuffle, neg, 4, chunk);
  size_t n = 0;
  for (;;) {
    const bool a = host.Next(), b = dev.Next();
    EXPECT(a == b, "part %d/%d shuffle %zu neg %g: batch %zu: host %d device %d", part, nparts,
           shuffle, neg, n, a, b);
    if (!a || !b) break;
    EXPECT(SameDeviceBatch(c, dstat, host.Value(), dev.Value()),
           "part %d/%d shuffle %zu neg %g: batch %zu differs", part, nparts, shuffle, neg, n);
    dev.Consumed();
    ++n;
    if (g_fail > 5) break;
  }
  if (fallback) *fallback = dev.FallbackChunks();
  return n;
}

int ModeBatches(dfx_ctx* c, const std::string& path, const std::string& dir) {
  Dev dstat(c, 32);
  const int64_t zero[4] = {0, 0, 0, 0};
  dstat.Up(zero, 32);
  const size_t bs = 257;
  DeviceTextFeed feed(c, bs, bs * 3);
  for (size_t shuffle : {(size_t)0, (size_t)3})
    for (float neg : {1.f, 0.7f})
      for (int pp = 0; pp < 2; ++pp) {
        const size_t n = CompareReaders(c, &dstat, &feed, path, pp, pp + 1, bs, shuffle, neg,
                                        64 << 10, nullptr);
        std::printf("batches part %d/%d shuffle %zu neg %g: %zu batches ok\n", pp, pp + 1,
                    shuffle, neg, n);
        EXPECT(n > 3, "too few batches");
      }
  {  // every chunk one batch (validation, prediction)
    TextReader host(path, "criteo", 0, 1, 256 << 10, 4);
    DeviceBatchReader dev(&feed, path, "criteo", 0, 1, 0, 0, 1.f, 4, 256 << 10);
    size_t n = 0;
    for (;;) {
      bool a;
      do {
        a = host.Next();
      } while (a && host.Value().Size() == 0);
      const bool b = dev.Next();
      EXPECT(a == b, "whole chunks: chunk %zu: host %d device %d", n, a, b);
      if (!a || !b) break;
      EXPECT(SameDeviceBatch(c, &dstat, host.Value(), dev.Value()), "whole chunk %zu differs", n);
      EXPECT(std::memcmp(dev.HostLabels(), host.Value().label.data(),
                         host.Value().Size() * 4) == 0,
             "whole chunk %zu: host labels differ", n);
      dev.Consumed();
      ++n;
    }
    std::printf("batches whole chunks: %zu ok\n", n);
    EXPECT(n > 3, "too few chunks");
  }
  {  // a file the device hands back: fractional labels, CRLF line ends
    const std::string bad = dir + "/needs_host.criteo";
    std::string text = GenRows(700, 9), out;
    for (size_t i = 0, line = 0; i < text.size(); ++i) {
      if (i == 0 || text[i - 1] == '\n') {
        ++line;
        if (line % 50 == 0) out += "0.5";
      }
      if (text[i] == '\n' && line % 77 == 0) out += '\r';
      out += text[i];
    }
    std::ofstream(bad, std::ios::binary) << out;
    size_t fb = 0;
    const size_t n = CompareReaders(c, &dstat, &feed, bad, 0, 1, bs, 3, 0.7f, 64 << 10, &fb);
    EXPECT(n > 0 && fb > 0, "needs_host file: %zu batches, %zu fallback chunks", n, fb);
    std::printf("batches needs_host file: %zu batches, %zu chunks parsed by the host ok\n", n, fb);
  }
  return 0;
}

// ---- CPU modes ---------------------------------------------------------------------------
bool SameHostBlock(const Block& a, const Block& b) {
  return a.Size() == b.Size() && a.offset == b.offset && a.index == b.index &&
         a.label.size() == b.label.size() &&
         (a.label.empty() ||
          std::memcmp(a.label.data(), b.label.data(), a.label.size() * 4) == 0);
}

int ModePlan(const std::string& path) {
  const size_t bs = 257, chunk = 64 << 10;
  for (size_t shuffle : {(size_t)0, (size_t)3})
    for (float neg : {1.f, 0.7f})
      for (int pp = 0; pp < 2; ++pp) {
        const int part = pp, nparts = pp + 1;
        BatchReader want(path, "criteo", part, nparts, bs, bs * shuffle, neg, 4, chunk);
        TextReader chunks(path, "criteo", part, nparts, chunk, 4);
        std::vector<Block> seq;  // the chunks by sequence number (the last one is live)
        Block shuf, batch;
        shuf.offset.assign(1, 0);
        BatchPlanner plan(
            bs, bs * shuffle, neg,
            [&](size_t* rows, const uint64_t** off, const float** lab) {
              if (!chunks.Next()) return false;
              seq.push_back(chunks.Value());
              *rows = seq.back().Size();
              *off = reinterpret_cast<const uint64_t*>(seq.back().offset.data());
              *lab = seq.back().label.data();
              return true;
            },
            [&](const GatherOp& op) {
              const Block& src = op.src == GatherOp::kShuffle ? shuf : seq[op.src];
              Block* dst = op.to_batch ? &batch : &shuf;
              if (!op.to_batch && op.r0 == 0) {
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
          EXPECT(SameHostBlock(want.Value(), batch),
                 "plan part %d/%d shuffle %zu neg %g: batch %zu differs", part, nparts, shuffle,
                 neg, n);
          ++n;
          if (g_fail > 5) break;
        }
        EXPECT(n > 3, "too few batches");
        std::printf("plan part %d/%d shuffle %zu neg %g: %zu batches ok\n", part, nparts,
                    shuffle, neg, n);
      }
  return 0;
}

int ModeCuts(const std::string& path, const std::string& dir) {
  // the same file without its last newline: the unterminated last line
  std::string text((std::istreambuf_iterator<char>(std::ifstream(path, std::ios::binary).rdbuf())),
                   std::istreambuf_iterator<char>());
  const std::string cut = dir + "/unterminated.criteo";
  std::ofstream(cut, std::ios::binary) << text.substr(0, text.size() - 1);
  for (const std::string& file : {path, cut})
    for (size_t chunk : {(size_t)4 << 10, (size_t)64 << 10, (size_t)1 << 20})
      for (int nparts : {1, 3})
        for (int part = 0; part < nparts; ++part)
          for (const char* fmt : {"criteo", "criteo_test"}) {
            TextReader parsed(file, fmt, part, nparts, chunk, 3);
            TextReader raw(file, fmt, part, nparts, chunk, 3);
            size_t n = 0, rows = 0;
            for (;;) {
              bool a;
              do {
                a = parsed.Next();
              } while (a && parsed.Value().Size() == 0);
              Block got;
              bool b;
              do {
                const char* data;
                size_t size;
                b = raw.NextRaw(&data, &size);
                got = Block();
                if (b) ParseCriteo(data, data + size, std::strcmp(fmt, "criteo") == 0, &got);
              } while (b && got.Size() == 0);
              EXPECT(a == b, "cuts chunk %zu part %d/%d: chunk %zu: parsed %d raw %d", chunk,
                     part, nparts, n, a, b);
              if (!a || !b) break;
              EXPECT(SameHostBlock(parsed.Value(), got), "cuts chunk %zu part %d/%d: chunk %zu",
                     chunk, part, nparts, n);
              rows += got.Size();
              ++n;
              if (g_fail > 5) return 1;
            }
            EXPECT(parsed.BytesRead() == raw.BytesRead(), "cuts: bytes read differ");
            if (nparts == 1) EXPECT(rows > 0, "cuts: no rows");
          }
  std::printf("cuts ok\n");
  return 0;
}

int ModeHashCells() {
  for (int len : kSweepLens)
    for (int j = 0; j < 39; ++j) {
      const std::string cell = SweepCell(len, j, 0);
      std::printf("%s\t%llu\n", cell.c_str(),
                  (unsigned long long)CityHash64(cell.data(), cell.size()));
    }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  const std::string a2 = argc > 2 ? argv[2] : "", a3 = argc > 3 ? argv[3] : "";
  if (mode == "hashcells") return ModeHashCells();
  if (mode == "plan" && argc > 2) {
    ModePlan(a2);
  } else if (mode == "cuts" && argc > 3) {
    ModeCuts(a2, a3);
  } else if (mode == "parse" || mode == "fallback" || mode == "gather" ||
             (mode == "batches" && argc > 3)) {
    dfx_ctx* c = nullptr;
    DfxCheck(dfx_ctx_create(0, "V_dim=0,max_keys=1024", &c), "dfx_ctx_create");
    if (mode == "parse") ModeParse(c);
    if (mode == "fallback") ModeFallback(c);
    if (mode == "gather") ModeGather(c);
    if (mode == "batches") ModeBatches(c, a2, a3);
    dfx_ctx_destroy(c);
  } else {
    std::fprintf(stderr,
                 "usage: %s parse | fallback | gather | batches FILE DIR | plan FILE | "
                 "cuts FILE DIR | hashcells\n",
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
