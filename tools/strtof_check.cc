// csrc/strtof.h against the host's strtof, bit for bit (CPU only).
//
//   strtof_check sample N SEED   random strings of every shape of the fast grammar: 1-19 digits,
//                                the point at every position, leading and trailing zeros,
//                                exponents making q every value in [-27, 27], both signs; one
//                                in eight is pushed just outside (q = +-28.., 20+ digits)
//   strtof_check edges           the ties, FLT_MAX and the first inf, the q = +-27 | 28 and
//                                19 | 20 digit boundaries, the not-fast forms; ids vs strtoull
//   strtof_check floats STRIDE   every STRIDE-th float bit pattern printed with %.9g
//
// Every "fast" answer must equal strtof's bits; a string is "fast" iff an independent matcher
// (in_grammar below, written over std::string, sharing nothing with the header) says it is in
// the grammar.  Prints the counts and ALL PASSED, exit status 0, or the differences and 1.
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../difacto_amd/csrc/strtof.h"

namespace {

uint32_t host_bits(const std::string& s, bool* whole) {
  char* end = nullptr;
  const float f = std::strtof(s.c_str(), &end);
  *whole = !s.empty() && end == s.c_str() + s.size();
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

// the grammar of csrc/strtof.h, restated: true iff s is in it (digit and q limits included)
bool in_grammar(const std::string& s) {
  size_t i = 0;
  if (i < s.size() && (s[i] == '+' || s[i] == '-')) ++i;
  const size_t m0 = i;
  while (i < s.size() && (isdigit((unsigned char)s[i]) || s[i] == '.')) ++i;
  const std::string mant = s.substr(m0, i - m0);
  const size_t dot = mant.find('.');
  if (dot != std::string::npos && mant.find('.', dot + 1) != std::string::npos) return false;
  const std::string ip = dot == std::string::npos ? mant : mant.substr(0, dot);
  const std::string fp = dot == std::string::npos ? "" : mant.substr(dot + 1);
  if (ip.empty() && fp.empty()) return false;
  long ex = 0;
  if (i < s.size()) {
    if (s[i] != 'e' && s[i] != 'E') return false;
    ++i;
    bool neg = false;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
    const std::string ed = s.substr(i);
    if (ed.empty() || ed.size() > 3) return false;
    for (char c : ed)
      if (!isdigit((unsigned char)c)) return false;
    ex = std::atol(ed.c_str());
    if (neg) ex = -ex;
  }
  std::string digits = ip + fp;
  const size_t nz = digits.find_first_not_of('0');
  if (nz == std::string::npos) return true;  // zero, whatever the exponent
  digits = digits.substr(nz);
  if (digits.size() > 19) return false;
  const long q = ex - (long)fp.size();
  return q >= -27 && q <= 27;
}

struct Tally {
  long n = 0, fast = 0, bad = 0;
  // checks one string; want_fast: -1 derive from in_grammar, 0 / 1 also assert it
  void check(const std::string& s, int want_fast = -1) {
    ++n;
    uint32_t got = 0;
    const bool isfast = dfx_strtof::parse(s.data(), (uint32_t)s.size(), &got);
    const bool gram = in_grammar(s);
    bool whole;
    const uint32_t ref = host_bits(s, &whole);
    bool ok = isfast == gram && (want_fast < 0 || isfast == (want_fast != 0));
    if (isfast) {
      ++fast;
      ok = ok && whole && got == ref;
    }
    if (!ok && ++bad <= 20)
      std::printf("DIFF '%s': fast %d (grammar %d, wanted %d) bits %08x strtof %08x whole %d\n",
                  s.c_str(), (int)isfast, (int)gram, want_fast, got, ref, (int)whole);
  }
};

uint64_t rng_state;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
int rint_in(int lo, int hi) { return lo + (int)(rnd() % (uint64_t)(hi - lo + 1)); }

std::string with_exp(const std::string& mant, long ex, bool force) {
  if (ex == 0 && !force && (rnd() & 1)) return mant;
  char buf[16];
  const char* fmt[] = {"%ld", "%02ld", "%03ld"};
  std::snprintf(buf, sizeof buf, fmt[rint_in(0, 2)], ex < 0 ? -ex : ex);
  std::string e = (rnd() & 1) ? "e" : "E";
  if (ex < 0) e += "-";
  else if (rnd() & 1) e += "+";
  return mant + e + buf;
}

int run_sample(long n, uint64_t seed) {
  rng_state = seed * 0x2545f4914f6cdd1dull + 1;
  Tally t;
  for (long it = 0; it < n; ++it) {
    const int nd = rint_in(1, 19);
    std::string d;
    for (int k = 0; k < nd; ++k) d += (char)('0' + rint_in(0, 9));
    if (rnd() % 3) d[0] = (char)('1' + rint_in(0, 8));      // mostly a non-zero lead
    if (rnd() % 4 == 0) for (int k = rint_in(1, nd); k < nd; ++k) d[k] = '0';  // trailing zeros
    bool outside = rnd() % 8 == 0;
    if (outside && d[0] == '0') outside = false;
    int q = rint_in(-27, 27);
    if (outside) {
      if (rnd() & 1) {
        q = (rnd() & 1) ? rint_in(28, 45) : -rint_in(28, 45);
      } else {
        while (d.size() < 20) d += (char)('0' + rint_in(0, 9));  // 20+ significant digits
      }
    }
    const int len = (int)d.size();
    const int zeros = rnd() % 4 == 0 ? rint_in(1, 6) : 0;
    std::string mant = std::string(zeros, '0') + d;
    int nfrac = 0;
    if (rnd() % 5) {  // the point at every position, the ends included
      nfrac = rint_in(0, len);
      mant.insert(mant.size() - nfrac, ".");
      if (zeros == 0 && nfrac == len && (rnd() & 1)) mant = "0" + mant;
    }
    std::string s = with_exp(mant, (long)q + nfrac, false);
    const int sg = rint_in(0, 3);
    if (sg == 1) s = "-" + s;
    if (sg == 2) s = "+" + s;
    bool allzero = d.find_first_not_of('0') == std::string::npos;
    t.check(s, allzero ? 1 : (outside ? 0 : 1));
  }
  std::printf("sample: %ld strings, %ld fast, %ld differences\n", t.n, t.fast, t.bad);
  return t.bad != 0;
}

int run_floats(long stride) {
  Tally t;
  char buf[64];
  for (uint64_t b = 0; b < (1ull << 32); b += (uint64_t)stride) {
    const uint32_t u = (uint32_t)b;
    float f;
    std::memcpy(&f, &u, 4);
    std::snprintf(buf, sizeof buf, "%.9g", f);
    t.check(buf);
    if (t.bad == 0 && in_grammar(buf)) {  // %.9g round-trips a float
      uint32_t got = 0;
      dfx_strtof::parse(buf, (uint32_t)std::strlen(buf), &got);
      if (got != u && ++t.bad <= 20) std::printf("DIFF '%s': no round trip of %08x\n", buf, u);
    }
  }
  std::printf("floats: %ld strings, %ld fast, %ld differences\n", t.n, t.fast, t.bad);
  return t.bad != 0;
}

int run_edges() {
  Tally t;
  const char* fast[] = {
      "16777217", "16777219", "33554434", "33554438", "8388608.5", "8388609.5", "0.1", "1",
      "1.0", "1e0", "1.0000001", "-1", "1e-27", "1e27",
      "9999999999999999999e27", "9999999999999999999e-27", "-0", "0", "+0.0", "0e99", "0e999",
      ".5", "5.", "+1", "-.5e1", "1e+05", "1E-3", "1.e5", "1234567890123456789",
      "0000000000000000000000000000001", "0.15", "0.3", "16777216", "16777215", "16777218",
      // FLT_MAX = 340282346638528859811704183484516925440; the tie to inf is
      // 340282356779733661637539395458142568448
      "3402823466385288598e20", "3402823567797336616e20", "3402823567797336617e20",
      "3402823567797336615e20", "340282350000000000e21", "340282360000000000e21",
      "340282350000e27", "340282360000e27", "3.4028235677973366e38",
      "-3402823567797336616e20", "1e20", "99999999999e27", "100000000000e27",
      "4294967296", "4294967295", "1844674407370955161",
      "9007199254740993", "123456789012345678.9",
      "0.9999999403953552", "0.99999997019767761", "0.99999994039535522",
  };
  const char* slow[] = {
      "3.4028235e38", "3.4028236e38", "0.34028236e39", "34028235e31", "18446744073709551615", "12345678901234567890", "1e28", "1e-28",
      "1.0000000000000000000e28", "0x1p3", "0x10", "inf", "-inf", "nan", "infinity", "1e", "1e+",
      "1.5abc", "", "+", "-", ".", "+.", "e5", "1e1234", "1..2", "1.2.3", " 1", "1 ", "1e5.0",
      "--1", "1,5", "1f", "1e-", "99999999999999999999",
  };
  for (const char* s : fast) t.check(s, 1);
  for (const char* s : slow) t.check(s, 0);
  // "3.4028235e38" / "3.4028236e38" have q = 38 - 7 = 31: outside; `fast` holds the |q| <= 27
  // spellings that reach FLT_MAX and the first inf.  0.000...01 with q = -27 | -28:
  t.check("0." + std::string(26, '0') + "1", 1);
  t.check("0." + std::string(27, '0') + "1", 0);
  t.check("000." + std::string(26, '0') + "10", 0);  // q counts the trailing zero: -28
  t.check("-." + std::string(26, '0') + "9", 1);
  t.check(std::string(40, '0') + "1", 1);
  t.check("1" + std::string(18, '0'), 1);  // 19 versus 20 significant digits
  t.check("1" + std::string(19, '0'), 0);
  t.check("1." + std::string(18, '0'), 1);
  t.check("1." + std::string(19, '0'), 0);
  // ids against strtoull: 19 and 20 digits, 2^64 - 1, 2^64 (saturates), 30 digits
  const char* ids[] = {"0", "7", "007", "1234567890123456789", "9999999999999999999",
                       "10000000000000000000", "18446744073709551615", "18446744073709551616",
                       "18446744073709551614", "18446744073709551620", "99999999999999999999",
                       "123456789012345678901234567890", "000000000000000000000000000042"};
  long idbad = 0;
  for (const char* s : ids) {
    uint64_t got = 0;
    errno = 0;
    const unsigned long long ref = std::strtoull(s, nullptr, 10);
    if (!dfx_strtof::parse_id(s, (uint32_t)std::strlen(s), &got) || got != ref) {
      ++idbad;
      std::printf("DIFF id '%s': %llu strtoull %llu\n", s, (unsigned long long)got, ref);
    }
  }
  uint64_t dummy;
  for (const char* s : {"", "12a", "+5", "-5", " 5", "0x5"})
    if (dfx_strtof::parse_id(s, (uint32_t)std::strlen(s), &dummy)) {
      ++idbad;
      std::printf("DIFF id '%s' accepted\n", s);
    }
  std::printf("edges: %ld strings, %ld fast, %ld differences; ids: %ld differences\n", t.n, t.fast,
              t.bad, idbad);
  return t.bad != 0 || idbad != 0;
}

}  // namespace

int main(int argc, char** argv) {
  int rc = 2;
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "sample" && argc == 4) rc = run_sample(std::atol(argv[2]), std::strtoull(argv[3], nullptr, 10));
  else if (mode == "edges") rc = run_edges();
  else if (mode == "floats" && argc == 3 && std::atol(argv[2]) > 0) rc = run_floats(std::atol(argv[2]));
  else std::fprintf(stderr, "usage: strtof_check sample N SEED | edges | floats STRIDE\n");
  if (rc == 0) std::printf("ALL PASSED\n");
  return rc;
}
