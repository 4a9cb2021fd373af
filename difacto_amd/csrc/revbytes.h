// include/difacto/base.h:39-51 - nibble reversal (involution).  A header of its own: one text
// for the kernels (common.h) and for host tools built without HIP (tools/modeltext_check.cc).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFX_REV_HD __host__ __device__ inline
#else
#define DFX_REV_HD inline
#endif

namespace dfx {

DFX_REV_HD uint64_t reverse_bytes(uint64_t x) {
  x = x << 32 | x >> 32;
  x = (x & 0x0000FFFF0000FFFFull) << 16 | (x & 0xFFFF0000FFFF0000ull) >> 16;
  x = (x & 0x00FF00FF00FF00FFull) << 8 | (x & 0xFF00FF00FF00FF00ull) >> 8;
  x = (x & 0x0F0F0F0F0F0F0F0Full) << 4 | (x & 0xF0F0F0F0F0F0F0F0ull) >> 4;
  return x;
}

}  // namespace dfx
