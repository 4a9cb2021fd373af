// gen_libsvm FILE ROWS SEED [nnz_lo nnz_hi id_bits style]
//
// Seeded libsvm rows "label id:value id:value ...\n" for the device parser's tests and
// measurements: a 0/1 label (30% ones), nnz uniform in [nnz_lo, nnz_hi] (default 39 39), ids
// uniform below 2^id_bits (default 24; 64: full 64-bit ids, 19 and 20 digits).
//   style 0   values printed with %g (6 digits)
//   style 1   values printed with %.15g, as rcv1's are
//   style 2   bare ids, no values
//   style 3   blocks of 1000 rows alternating between style 0 and all-ones rows (bare ids,
//             ":1", ":1.0", ":1e0" in turn), so that readers form valued and binary batches
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s FILE ROWS SEED [nnz_lo nnz_hi id_bits style]\n", argv[0]);
    return 2;
  }
  const long rows = std::atol(argv[2]);
  const unsigned long long seed = std::strtoull(argv[3], nullptr, 10);
  const int nnz_lo = argc > 4 ? std::atoi(argv[4]) : 39;
  const int nnz_hi = argc > 5 ? std::atoi(argv[5]) : nnz_lo;
  const int id_bits = argc > 6 ? std::atoi(argv[6]) : 24;
  const int style = argc > 7 ? std::atoi(argv[7]) : 0;
  if (rows < 0 || nnz_lo < 0 || nnz_hi < nnz_lo || id_bits < 1 || id_bits > 64 || style < 0 ||
      style > 3) {
    std::fprintf(stderr, "gen_libsvm: bad argument\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) {
    std::fprintf(stderr, "gen_libsvm: cannot open %s\n", argv[1]);
    return 1;
  }
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const uint64_t mask = id_bits == 64 ? ~0ull : (1ull << id_bits) - 1;
  static const char* const ones[] = {"", ":1", ":1.0", ":1e0"};
  std::string line;
  char buf[64];
  for (long r = 0; r < rows; ++r) {
    line = U(rng) < 0.3 ? "1" : "0";
    const int nnz = nnz_lo + (int)(rng() % (uint64_t)(nnz_hi - nnz_lo + 1));
    int st = style;
    if (style == 3) st = (r / 1000) % 2 ? 4 : 0;
    for (int j = 0; j < nnz; ++j) {
      std::snprintf(buf, sizeof buf, " %llu", (unsigned long long)(rng() & mask));
      line += buf;
      const double v = 0.001 + 0.998 * U(rng);
      if (st == 0) {
        std::snprintf(buf, sizeof buf, ":%g", v);
        line += buf;
      } else if (st == 1) {
        std::snprintf(buf, sizeof buf, ":%.15g", v);
        line += buf;
      } else if (st == 4) {
        line += ones[(r + j) % 4];
      }
    }
    line += '\n';
    std::fwrite(line.data(), 1, line.size(), f);
  }
  return std::fclose(f) == 0 ? 0 : 1;
}
