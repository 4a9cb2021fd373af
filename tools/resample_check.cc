// csrc/reshuffle.h's per-epoch down-sample from the host (CPU only): pins rs_draw and rs_dropped
// to their numpy restatement (tests/resample_ref.py) without a GPU.
//
//   resample_check N KEY NEG_SAMPLING    for every source row 0 .. N - 1 with label 0: the bits of
//                                        rs_draw(KEY, row) as a decimal uint32 and rs_dropped's
//                                        flag, "bits flag" a line
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../difacto_amd/csrc/reshuffle.h"

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: resample_check N KEY NEG_SAMPLING\n");
    return 2;
  }
  const unsigned long long n = std::strtoull(argv[1], nullptr, 10);
  const uint64_t key = std::strtoull(argv[2], nullptr, 10);
  const float neg_sampling = std::strtof(argv[3], nullptr);
  if (n >= (1ull << 31)) {
    std::fprintf(stderr, "N must be below 2^31\n");
    return 2;
  }
  std::string out;
  out.reserve((size_t)n * 14 + 16);
  char buf[32];
  for (uint32_t row = 0; row < (uint32_t)n; ++row) {
    const float u = rs_draw(key, row);
    uint32_t bits;
    std::memcpy(&bits, &u, 4);
    const int len = std::snprintf(buf, sizeof buf, "%u %d\n", bits,
                                  rs_dropped(key, row, 0.f, neg_sampling) ? 1 : 0);
    out.append(buf, (size_t)len);
  }
  std::fwrite(out.data(), 1, out.size(), stdout);
  return 0;
}
