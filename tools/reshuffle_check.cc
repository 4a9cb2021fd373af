// csrc/reshuffle.h from the host (CPU only): pins the header to its numpy restatement
// (tests/reshuffle_ref.py) without a GPU.
//
//   reshuffle_check N KEY                    prints rs_perm(j, N, KEY) for j = 0 .. N - 1, one
//                                            number a line
//   reshuffle_check key SEED EPOCH LIST      prints rs_epoch_key(SEED, EPOCH, LIST)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../difacto_amd/csrc/reshuffle.h"

int main(int argc, char** argv) {
  if (argc == 5 && std::strcmp(argv[1], "key") == 0) {
    std::printf("%llu\n", (unsigned long long)rs_epoch_key(std::strtoull(argv[2], nullptr, 10),
                                                          std::strtoull(argv[3], nullptr, 10),
                                                          std::strtoull(argv[4], nullptr, 10)));
    return 0;
  }
  if (argc != 3) {
    std::fprintf(stderr, "usage: reshuffle_check N KEY | key SEED EPOCH LIST\n");
    return 2;
  }
  const unsigned long long n = std::strtoull(argv[1], nullptr, 10);
  const uint64_t key = std::strtoull(argv[2], nullptr, 10);
  if (n >= (1ull << 31)) {
    std::fprintf(stderr, "N must be below 2^31\n");
    return 2;
  }
  const rs_net t = rs_make((uint32_t)n, key);
  std::string out;
  out.reserve((size_t)n * 8 + 16);
  char buf[16];
  for (uint32_t j = 0; j < (uint32_t)n; ++j) {
    const int len = std::snprintf(buf, sizeof buf, "%u\n", rs_apply(t, j));
    out.append(buf, (size_t)len);
  }
  std::fwrite(out.data(), 1, out.size(), stdout);
  return 0;
}
