// Lane helpers of the FM kernels shared by fm.hip, fm_line.hip and fm_half.hip: a lane's
// coordinates of a row, an occurrence's p, a lane's 16-byte piece of fp16 values.
#pragma once
#include <algorithm>

#include "fm_args.h"

namespace dfx {

constexpr int kFmNT = 256;

// Coordinates [l*CPL, l*CPL+CPL) of a length-d row.  VEC: d is a multiple of the vector
// width and the row 16-byte aligned, so a lane's chunk is wholly inside or wholly outside
// the row (outside chunks read chunk 0 and are ignored).
template <int CPL, bool VEC>
__device__ inline void load_coords(const float* row, int l, int d, float (&v)[CPL],
                                   bool nt = false) {
  const int base = l * CPL;
  if constexpr (VEC && CPL % 4 == 0) {
    const int b = base < d ? base : 0;
#pragma unroll
    for (int m = 0; m < CPL / 4; ++m) {
      const float4 f = ld4(row + b + 4 * m, nt);
      v[4 * m] = f.x; v[4 * m + 1] = f.y; v[4 * m + 2] = f.z; v[4 * m + 3] = f.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int cd = base + k;
      v[k] = ldnt(row + (cd < d ? cd : 0), nt);
    }
  }
}

template <int CPL, bool VEC>
__device__ inline void store_coords(float* row, int l, int d, const float (&v)[CPL],
                                    bool nt = false) {
  const int base = l * CPL;
  if (base >= d) return;
  if constexpr (VEC && CPL % 4 == 0) {
#pragma unroll
    for (int m = 0; m < CPL / 4; ++m)
      st4(row + base + 4 * m, make_float4(v[4 * m], v[4 * m + 1], v[4 * m + 2], v[4 * m + 3]),
          nt);
  } else {
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      if (base + k < d) stnt(row + base + k, v[k], nt);
  }
}

// p of row r for a backward that also reads the row's XV*p: from the XV*p row when p shares
// its last line (4d % 128 != 0: d = 16's 68 bytes in one 128-byte line), else from the
// compact per-row array (d = 64 / 128: p would be a line of its own in a 384 / 640-byte row,
// where the 400-KB array stays in the L2); the split owner has only the rows (p == nullptr)
__device__ inline float row_p(const BwdArgs& a, uint32_t r, int d, int64_t xs) {
  if (a.p && (xs <= d || (4 * d) % 128 == 0)) return a.p[r];
  return a.XVp[(int64_t)r * xs + d];
}

// ---- 16-byte pieces of fp16 bit patterns (half rows, fm_half.hip; line slots at d = 24,
// fm_line.hip) -----------------------------------------------------------------------------------
typedef uint32_t dfx_u4v __attribute__((ext_vector_type(4)));

// a lane's 16-byte piece of a half row: eight fp16 bit patterns, coordinate k in the low half of
// word k / 2 for even k
__device__ __forceinline__ dfx_u4v ldh(const uint16_t* p, bool nt) {
  const dfx_u4v* q = reinterpret_cast<const dfx_u4v*>(p);
  return nt ? __builtin_nontemporal_load(q) : *q;
}
__device__ __forceinline__ void sth(uint16_t* p, dfx_u4v v, bool nt) {
  dfx_u4v* q = reinterpret_cast<dfx_u4v*>(p);
  if (nt) __builtin_nontemporal_store(v, q);
  else *q = v;
}
__device__ __forceinline__ void half8_widen(dfx_u4v p, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = f16_widen(p[i] & 0xFFFFu);
    f[2 * i + 1] = f16_widen(p[i] >> 16);
  }
}
__device__ __forceinline__ dfx_u4v half8_pack(const uint32_t (&h)[8]) {
  dfx_u4v p;
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = h[2 * i] | (h[2 * i + 1] << 16);
  return p;
}

// a resident grid for kernel K (its groups loop over rows): at most want blocks
template <typename K>
inline int64_t resident_grid_for(K kern, int64_t want) {
  int per_cu = 0, dev = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kFmNT, 0) != hipSuccess ||
      per_cu <= 0 || hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus <= 0)
    return want;
  return std::min<int64_t>(want, (int64_t)per_cu * cus);
}

}  // namespace dfx
