// gen_adfea FILE ROWS SEED [nnz_lo nnz_hi id_bits groups]
//
// Seeded adfea rows "lineid count label idx:gid idx:gid ...\n" (src/reader/adfea_parser.h) for
// the device parser's tests and measurements, all inside the domain dfx_parse_adfea parses on
// the device: a 0/1 label (30% ones), nnz uniform in [nnz_lo, nnz_hi] (default 39 39: Criteo's
// row length), idx uniform below 2^id_bits (default 24; 64: full 64-bit ids, whose top 12 bits
// the encoding shifts out), gid uniform below groups (default 39, at most 4096).  Blanks are
// mixed: mostly one space, now and then a tab, two spaces, a blank before the lineid or before
// the '\n'.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s FILE ROWS SEED [nnz_lo nnz_hi id_bits groups]\n", argv[0]);
    return 2;
  }
  const long rows = std::atol(argv[2]);
  const unsigned long long seed = std::strtoull(argv[3], nullptr, 10);
  const int nnz_lo = argc > 4 ? std::atoi(argv[4]) : 39;
  const int nnz_hi = argc > 5 ? std::atoi(argv[5]) : nnz_lo;
  const int id_bits = argc > 6 ? std::atoi(argv[6]) : 24;
  const int groups = argc > 7 ? std::atoi(argv[7]) : 39;
  if (rows < 0 || nnz_lo < 0 || nnz_hi < nnz_lo || id_bits < 1 || id_bits > 64 || groups < 1 ||
      groups > 4096) {
    std::fprintf(stderr, "gen_adfea: bad argument\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "wb");
  if (!f) {
    std::fprintf(stderr, "gen_adfea: cannot open %s\n", argv[1]);
    return 1;
  }
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const uint64_t mask = id_bits == 64 ? ~0ull : (1ull << id_bits) - 1;
  std::string line;
  char buf[64];
  const auto blank = [&]() {
    const uint64_t k = rng() % 16;
    line += k == 0 ? "\t" : k == 1 ? "  " : k == 2 ? " \t" : " ";
  };
  for (long r = 0; r < rows; ++r) {
    line.clear();
    if (rng() % 32 == 0) line += rng() % 2 ? " " : "\t";
    const int nnz = nnz_lo + (int)(rng() % (uint64_t)(nnz_hi - nnz_lo + 1));
    std::snprintf(buf, sizeof buf, "%ld", r);
    line += buf;
    blank();
    std::snprintf(buf, sizeof buf, "%d", nnz);
    line += buf;
    blank();
    line += U(rng) < 0.3 ? "1" : "0";
    for (int j = 0; j < nnz; ++j) {
      blank();
      std::snprintf(buf, sizeof buf, "%llu:%d", (unsigned long long)(rng() & mask),
                    (int)(rng() % (uint64_t)groups));
      line += buf;
    }
    if (rng() % 32 == 0) line += rng() % 2 ? " " : "\t";
    line += '\n';
    std::fwrite(line.data(), 1, line.size(), f);
  }
  return std::fclose(f) == 0 ? 0 : 1;
}
