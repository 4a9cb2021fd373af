// csrc/fmtg.h against the host's snprintf("%g"), byte for byte (CPU only).
//
//   fmtg_check floats STRIDE    every STRIDE-th float bit pattern as a raw prediction
//   fmtg_check probs STRIDE     the same floats through the probability; the header's double
//                               against the host expression's bits, then its text
//   fmtg_check sample N SEED    doubles log-uniform over [1e-13, 1e13), both signs: the
//                               guaranteed domain and a decade beyond each end
//   fmtg_check edges            the %e / %f switches at 1e-5, 1e-4, 999999.5 and 1e6, exact
//                               six-digit ties both ways, 0.5, the zeros, subnormals,
//                               non-finite values, both ends of the guaranteed domain
//   fmtg_check rows IN OUT      IN: binary (float label, float pred) pairs.  OUT.p0 / OUT.p1: the
//                               driver's fprintf of every row with pred_prob 0 / 1; OUT.v0 /
//                               OUT.v1: the doubles it printed (binary).  The expected text of
//                               the GPU tests (numpy's exp is not glibc's expf).
//   fmtg_check edgelist OUT     the edges' values as binary floats (inputs for those tests)
//
// Every output is identical or flagged (needs host); inside the guaranteed domain, +-0 and
// 1e-12 <= |x| < 1e12, nothing is flagged.  Prints the counts and ALL PASSED, exit status 0, or
// the differences and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../difacto_amd/csrc/fmtg.h"

namespace {

const uint64_t kTab[32] = DFX_EXP2F_TAB;
uint64_t Tab(int i) { return kTab[i]; }

long g_checked = 0, g_flagged = 0, g_bad = 0;

bool Guaranteed(double x) {
  const double a = std::fabs(x);
  return a == 0.0 || (a >= 1e-12 && a < 1e12);
}

void CheckOne(double x) {
  char want[64], got[dfx_fmtg::kRecBytes];
  const int wn = std::snprintf(want, sizeof(want), "%g", x);
  const int gn = dfx_fmtg::fmt_g(x, got);
  ++g_checked;
  if (gn < 0) {
    ++g_flagged;
    if (Guaranteed(x)) {
      if (++g_bad <= 20) std::printf("FLAGGED in the guaranteed domain: %a (%s)\n", x, want);
    }
    return;
  }
  if (gn > dfx_fmtg::kMaxField || gn != wn || std::memcmp(want, got, wn) != 0) {
    if (++g_bad <= 20) std::printf("DIFF %a: host '%s' header '%.*s'\n", x, want, gn, got);
  }
}

float FromBits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

// the driver's expression (train_main.cc WritePredRows)
double HostValue(float pred, bool prob) {
  return prob ? 1.0 / (1.0 + std::exp(-pred)) : (double)pred;
}

int Finish(const char* what) {
  std::printf("%s: %ld checked, %ld flagged, %ld bad\n", what, g_checked, g_flagged, g_bad);
  if (g_bad) return 1;
  std::printf("ALL PASSED\n");
  return 0;
}

std::vector<float> EdgeFloats() {
  std::vector<float> v = {0.f,     -0.f,    0.5f,     -0.5f,   1.f,      -1.f,     3.f,
                          20.f,    -20.f,   1e-5f,    1e-4f,   9.99995e-5f, 999999.5f, 1e6f,
                          999999.f, 123456.5f, 123457.5f, 0.25f, 1e-12f,  1e11f,    9.99999e11f,
                          1e-30f,  1e30f,   88.f,     -88.f,   103.f,    -103.f,   17.f,
                          -17.f,   1e-7f,   12345.67f, 0.001f, 0.0001234565f};
  for (uint32_t b : {0x00000001u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0x7f800000u,
                     0xff800000u, 0x7fc00000u, 0xffc00000u})
    v.push_back(FromBits(b));
  return v;
}

int Edges() {
  std::vector<double> v;
  for (float f : EdgeFloats()) v.push_back((double)f);
  // the style switches and their neighbours
  for (double x : {1e-5, 1e-4, 999999.5, 1e6, 9.999995e-5, 9.9999949999e-5, 99999.95, 999999.4999,
                   1e-12, 1e12, 0.5, 1.5, 2.5, 1e5, 100000.5, 1e-4 * 0.99999949, 5e-324,
                   2.2250738585072014e-308, 1.7976931348623157e308, 1e22, 1e-13, 1e-14})
    for (double y : {x, std::nextafter(x, 0.0), std::nextafter(x, 1e300)})
      for (double s : {1.0, -1.0}) v.push_back(s * y);
  // exact six-digit ties: d.ddddd5 * 2^j forms that are exact in binary (round half to even
  // both ways), 100000.5 .. 999999.5 in steps and scaled by powers of two
  for (int i = 0; i < 2000; ++i) {
    const double t = 100000.5 + 449.0 * i;  // exact: an integer plus one half
    v.push_back(t);
    v.push_back(-t);
    v.push_back(t / 8);       // ddddd.dd 0625: exact, below a tie
    v.push_back(t + 1.0);
  }
  for (int i = 0; i < 64; ++i) {
    v.push_back((1000005.0 + 20.0 * i));        // d.ddddd|5 at seven digits: ties of 1e6..
    v.push_back((1000015.0 + 20.0 * i) * 10);   // 1000015 * 10: tie at eight digits
    v.push_back((double)(1000005 + 20 * i) * 1000.0);
  }
  const double lo = 1e-12, hi = 1e12;
  v.push_back(lo);
  v.push_back(std::nextafter(hi, 0.0));
  v.push_back(-lo);
  v.push_back(-std::nextafter(hi, 0.0));
  for (double x : v) CheckOne(x);
  return Finish("edges");
}

int Floats(uint32_t stride, bool probs) {
  long value_bad = 0;
  for (uint64_t b = 0; b < (1ull << 32); b += stride) {
    const float f = FromBits((uint32_t)b);
    const double want = HostValue(f, probs), got = dfx_fmtg::pred_value(f, probs ? 1 : 0, Tab);
    if (std::memcmp(&want, &got, 8) != 0 && !(want != want && got != got)) {
      if (++value_bad <= 20) std::printf("VALUE %a: host %a header %a\n", (double)f, want, got);
    }
    CheckOne(got);
  }
  g_bad += value_bad;
  return Finish(probs ? "probs" : "floats");
}

uint64_t SplitMix(uint64_t* s) {
  *s += 0x9E3779B97F4A7C15ull;
  uint64_t z = *s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int Sample(long n, uint64_t seed) {
  uint64_t s = seed;
  for (long i = 0; i < n; ++i) {
    const uint64_t r = SplitMix(&s);
    const double u = (double)(r >> 11) / 9007199254740992.0;  // [0, 1)
    double x = std::pow(10.0, -13.0 + 26.0 * u);
    if (SplitMix(&s) & 1) x = -x;
    CheckOne(x);
  }
  return Finish("sample");
}

bool WriteAll(const std::string& path, const void* p, size_t n) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(p, 1, n, f) == n;
  return std::fclose(f) == 0 && ok;
}

int Rows(const char* in, const std::string& out) {
  FILE* f = std::fopen(in, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", in);
    return 1;
  }
  std::vector<float> lp;
  float buf[2];
  while (std::fread(buf, 4, 2, f) == 2) {
    lp.push_back(buf[0]);
    lp.push_back(buf[1]);
  }
  std::fclose(f);
  const size_t n = lp.size() / 2;
  for (int prob = 0; prob < 2; ++prob) {
    FILE* pf = std::fopen((out + (prob ? ".p1" : ".p0")).c_str(), "w");
    if (!pf) return 1;
    std::vector<double> vals(n);
    for (size_t i = 0; i < n; ++i) {
      const float label = lp[2 * i], pred = lp[2 * i + 1];
      vals[i] = HostValue(pred, prob != 0);
      std::fprintf(pf, "%g\t%g\n", label, prob ? 1.0 / (1.0 + std::exp(-pred)) : (double)pred);
    }
    if (std::fclose(pf) != 0) return 1;
    if (!WriteAll(out + (prob ? ".v1" : ".v0"), vals.data(), n * 8)) return 1;
  }
  std::printf("rows: %zu\n", n);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "edges" && argc == 2) return Edges();
  if ((mode == "floats" || mode == "probs") && argc == 3 && std::atol(argv[2]) > 0)
    return Floats((uint32_t)std::atol(argv[2]), mode == "probs");
  if (mode == "sample" && argc == 4)
    return Sample(std::atol(argv[2]), std::strtoull(argv[3], nullptr, 10));
  if (mode == "rows" && argc == 4) return Rows(argv[2], argv[3]);
  if (mode == "edgelist" && argc == 3) {
    const std::vector<float> v = EdgeFloats();
    return WriteAll(argv[2], v.data(), v.size() * 4) ? 0 : 1;
  }
  std::fprintf(stderr,
               "usage: fmtg_check floats STRIDE | probs STRIDE | sample N SEED | edges | "
               "rows IN OUT | edgelist OUT\n");
  return 2;
}
