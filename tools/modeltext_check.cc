// Test infrastructure: csrc/modeltext.h (the device model dump's lines) against a real
// std::ostream, which is what SGDUpdater::Dump (src/sgd/sgd_updater.h:108-139) and
// dfx_store_dump print through.  Plain g++, no HIP.
//
//   modeltext_check keys                      the edge keys, as stored and nibble-reversed: fmt_u64
//                                             against operator<<, reverse_bytes an involution;
//                                             "key K rev R length L" for each
//   modeltext_check lens                      "L value length" for the least and the greatest
//                                             key of every decimal length L = 1..20
//   modeltext_check lines N SEED D AUX REV EDGES
//                                             N random entries whose floats come from EDGES (the
//                                             binary floats of `fmtg_check edgelist`) and from
//                                             random bit patterns: a line whose floats are all
//                                             +-0 or 1e-12 <= |x| < 1e12 must be the stream's
//                                             bytes; one with a float that is not finite, a
//                                             float subnormal, below 1e-15 or from 1e12 must
//                                             answer "needs host"; in between either, and never
//                                             other bytes
// Every mode prints a summary line and exits 0 only when nothing differed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../difacto_amd/csrc/modeltext.h"

namespace mt = dfx_modeltext;

static const uint64_t kEdgeKeys[] = {0ull, 1ull, 9ull, 10ull, 99ull, 9999999999999999999ull,
                                     10000000000000000000ull, 1ull << 63, ~0ull - 1};

static std::string stream_u64(uint64_t v) {
  std::ostringstream os;
  os << v;
  return os.str();
}

static int run_keys() {
  int bad = 0, n = 0;
  for (uint64_t k : kEdgeKeys) {
    if (dfx::reverse_bytes(dfx::reverse_bytes(k)) != k) ++bad;
    for (int rev = 0; rev < 2; ++rev) {
      char buf[mt::kFieldBytes];
      const uint64_t p = mt::printed_key(k, rev);
      const int L = mt::fmt_u64(p, buf);
      const std::string want = stream_u64(rev ? dfx::reverse_bytes(k) : k);
      if (L != (int)want.size() || memcmp(buf, want.data(), want.size()) != 0) {
        ++bad;
        printf("key %llu rev %d: got %.*s want %s\n", (unsigned long long)k, rev, L, buf,
               want.c_str());
      }
      printf("key %llu rev %d length %d\n", (unsigned long long)k, rev, L);
      ++n;
    }
  }
  printf("keys: %d checked, %d differ\n", n, bad);
  return bad ? 1 : 0;
}

static int run_lens() {
  int bad = 0;
  uint64_t lo = 1;
  for (int L = 1; L <= 20; ++L) {
    const uint64_t first = L == 1 ? 0 : lo;
    const uint64_t last = L == 20 ? ~0ull : lo * 10 - 1;
    for (uint64_t v : {first, last}) {
      char buf[mt::kFieldBytes];
      const int n = mt::fmt_u64(v, buf);
      const std::string want = stream_u64(v);
      if (n != (int)want.size() || memcmp(buf, want.data(), want.size()) != 0) ++bad;
      printf("%d %llu %d\n", L, (unsigned long long)v, n);
    }
    if (L < 20) lo *= 10;
  }
  printf("lens: %d differ\n", bad);
  return bad ? 1 : 0;
}

static bool guaranteed(float f) {
  const double a = std::fabs((double)f);
  return a == 0 || (a >= 1e-12 && a < 1e12);
}
static bool refused(float f) {
  const double a = std::fabs((double)f);
  return !std::isfinite(f) || (a != 0 && (std::fpclassify(f) == FP_SUBNORMAL || a < 1e-15 ||
                                          a >= 1e12));
}

static int run_lines(int64_t N, uint64_t seed, int d, int aux, int rev, const char* edges_path) {
  std::vector<float> edges;
  if (FILE* f = fopen(edges_path, "rb")) {
    float x;
    while (fread(&x, 4, 1, f) == 1) edges.push_back(x);
    fclose(f);
  }
  if (edges.empty()) {
    fprintf(stderr, "no floats in %s\n", edges_path);
    return 2;
  }
  std::vector<float> safe;
  for (float x : edges)
    if (guaranteed(x)) safe.push_back(x);
  std::mt19937_64 rng(seed);
  auto draw = [&](bool any) -> float {
    const uint64_t r = rng();
    const int pick = (int)(r & 3);
    if (pick == 0 && any) return edges[(r >> 8) % edges.size()];
    if (pick == 1) return safe[(r >> 8) % safe.size()];
    if (pick == 2 && any) {  // any bit pattern
      const uint32_t b = (uint32_t)(r >> 20);
      float x;
      memcpy(&x, &b, 4);
      return x;
    }
    // a float of a random decimal magnitude inside the guaranteed domain
    const double mag = std::pow(10.0, -12.0 + 24.0 * (double)((r >> 8) & 0xFFFFF) / 1048576.0);
    const float x = (float)((r >> 40 & 1) ? -mag : mag);
    return guaranteed(x) ? x : 1.f;
  };
  int64_t same = 0, host = 0, differ = 0, longest = 0;
  std::vector<char> out((size_t)mt::worst_line_bytes(d, aux) + 64);
  std::vector<float> V((size_t)d), C((size_t)d);
  for (int64_t i = 0; i < N; ++i) {
    const bool any = (rng() % 10) < 3;  // 3 entries of 10 may hold floats outside the domain
    const uint64_t key = i < 9 ? kEdgeKeys[i] : rng();
    const bool has_v = d > 0 && (rng() & 1);
    const float w = draw(any), sg = draw(any), z = draw(any);
    for (int k = 0; k < d; ++k) {
      V[k] = draw(any);
      C[k] = draw(any);
    }
    std::ostringstream os;
    os << (rev ? dfx::reverse_bytes(key) : key) << '\t' << (has_v ? 1 + d : 1) << '\t' << w;
    if (aux) os << '\t' << sg << '\t' << z;
    bool all_ok = guaranteed(w), must_refuse = refused(w);
    auto see = [&](float x) {
      all_ok = all_ok && guaranteed(x);
      must_refuse = must_refuse || refused(x);
    };
    if (aux) { see(sg); see(z); }
    if (has_v) {
      for (int k = 0; k < d; ++k) { os << '\t' << V[k]; see(V[k]); }
      if (aux)
        for (int k = 0; k < d; ++k) { os << '\t' << C[k]; see(C[k]); }
    }
    os << '\n';
    const std::string want = os.str();
    const int64_t L = mt::fmt_line(key, rev, w, sg, z, has_v ? V.data() : nullptr,
                                   has_v ? C.data() : nullptr, d, aux, out.data());
    if (L < 0) {
      ++host;
      if (all_ok) {
        ++differ;
        printf("entry %lld: refused, want %s", (long long)i, want.c_str());
      }
      continue;
    }
    if (must_refuse || L != (int64_t)want.size() || memcmp(out.data(), want.data(), (size_t)L)) {
      ++differ;
      printf("entry %lld: got %.*s want %s", (long long)i, (int)L, out.data(), want.c_str());
      continue;
    }
    if (L > mt::worst_line_bytes(d, aux)) ++differ;
    longest = L > longest ? L : longest;
    ++same;
  }
  printf("lines: %lld equal, %lld need the host, %lld differ, longest %lld of %lld\n",
         (long long)same, (long long)host, (long long)differ, (long long)longest,
         (long long)mt::worst_line_bytes(d, aux));
  return differ ? 1 : 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "keys" && argc == 2) return run_keys();
  if (mode == "lens" && argc == 2) return run_lens();
  if (mode == "lines" && argc == 8)
    return run_lines(atoll(argv[2]), strtoull(argv[3], nullptr, 10), atoi(argv[4]), atoi(argv[5]),
                     atoi(argv[6]), argv[7]);
  fprintf(stderr, "usage: modeltext_check keys | lens | lines N SEED D AUX REV EDGES\n");
  return 2;
}
