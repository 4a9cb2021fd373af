// csrc/vhalf.h and csrc/vaux16.h as the host compiles them (CPU only; test infrastructure).
//
//   half_round_check FILE    FILE: binary tuples of four uint32 {bits of nv, bits of g, bits of sg,
//                            j}.  Prints per tuple, in hex, vhalf_round(nv, g, sg, j),
//                            vaux16_round(|nv|, g, sg, j) and f16_nearest(nv) — what
//                            dfx_half_round_table returns from the device.
// tests/test_gpu_half_paths.py compares the lines with the numpy yardstick.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define __host__
#define __device__
#include "../../difacto_amd/csrc/vhalf.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: half_round_check FILE\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<uint32_t> in;
  uint32_t t[4];
  while (std::fread(t, sizeof(uint32_t), 4, f) == 4) in.insert(in.end(), t, t + 4);
  std::fclose(f);
  for (size_t i = 0; i + 3 < in.size(); i += 4) {
    const float nv = dfx::bits_f32(in[i]), g = dfx::bits_f32(in[i + 1]);
    const float sg = dfx::bits_f32(in[i + 2]);
    const int j = (int)in[i + 3];
    std::printf("%x %x %x\n", dfx::vhalf_round(nv, g, sg, j),
                dfx::vaux16_round(dfx::bits_f32(in[i] & 0x7FFFFFFFu), g, sg, j),
                dfx::f16_nearest(nv));
  }
  return 0;
}
