// Half-precision Vaux (kwarg slot_layout=line vaux=f16, V_dim 16): the fp16 bit patterns a line
// slot stores for the AdaGrad accumulators, and the one rounding every Update goes through.
// Integer and exact fp32 operations only, the same on the host and the device (no fp16 type, no
// conversion instruction, no denormal mode): tests/line16_ref.py restates them in numpy.
#pragma once
#include <cstdint>
#include <cstring>

namespace dfx {

constexpr uint32_t kF16Max = 0x7BFFu;  // 65504, the largest finite fp16

__host__ __device__ inline uint32_t f32_bits(float x) {
  uint32_t b;
  memcpy(&b, &x, 4);
  return b;
}
__host__ __device__ inline float bits_f32(uint32_t b) {
  float x;
  memcpy(&x, &b, 4);
  return x;
}

// an fp16 bit pattern widened, exactly (subnormals included)
__host__ __device__ inline float f16_widen(uint32_t h) {
  const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
  if (e == 0) return bits_f32(s | f32_bits((float)m * 5.9604644775390625e-08f));  // m * 2^-24
  return bits_f32(s | ((e == 31 ? 255u : e + 112u) << 23) | (m << 13));
}

// 0 <= x < 65504: the largest fp16 <= x (lo; the next fp16 is lo + 1, across the subnormal
// boundary too) and fr = 8192 * (x - lo) / (hi - lo), exact: hi - lo is a power of two.  A
// normal fp16 drops 13 mantissa bits, which are fr; below 2^-14 the fp16 grid is 2^-24
__host__ __device__ inline uint32_t f16_floor(float x, float* fr) {
  const uint32_t b = f32_bits(x), e = b >> 23;
  if (e >= 113u) {  // x >= 2^-14
    *fr = (float)(b & 0x1FFFu);
    return ((e - 112u) << 10) | ((b >> 13) & 1023u);
  }
  const float t = x * 16777216.f;  // x * 2^24 < 1024
  const uint32_t lo = (uint32_t)t;
  *fr = (t - (float)lo) * 8192.f;
  return lo;
}

// the nearest fp16, ties to even, saturating at +-65504 (a NaN reads as too large): what a
// model file's fp32 Vaux becomes in a line16 slot — exact for a file such a slot wrote
__host__ __device__ inline uint32_t f16_nearest(float x) {
  const uint32_t s = (f32_bits(x) >> 16) & 0x8000u;
  const float ax = bits_f32(f32_bits(x) & 0x7FFFFFFFu);
  if (!(ax < 65504.f)) return s | kF16Max;
  float fr;
  const uint32_t lo = f16_floor(ax, &fr);
  return s | (lo + ((fr > 4096.f || (fr == 4096.f && (lo & 1u))) ? 1u : 0u));
}

__host__ __device__ inline uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// The stored fp16 of a new accumulator nc = sqrtf(c c + g g) (adagrad_update), rounded
// stochastically with random bits that are a hash of the operands' own bits: g the regularised
// gradient, sg the key's sqrt_g after the UpdateW of the same Update, j the coordinate.
// Nearest rounding stalls a hot key's accumulator (once g g is under half an ulp of c the sum
// never moves: DESIGN.md "Line slots at V_dim 16"); this one is unbiased over the hash and a
// pure function of the update, so a run stays reproducible bit for bit.
//   nc >= 65504 (or NaN): 65504, saturating — no inf is stored
//   else lo <= nc < hi neighbouring fp16, f = (nc - lo) / (hi - lo), r = 13 hash bits:
//   hi iff f * 8192 > r — a value that is an fp16 already (f = 0) is stored as it is
__host__ __device__ inline uint32_t vaux16_round(float nc, float g, float sg, int j) {
  if (!(nc < 65504.f)) return kF16Max;
  float fr;
  const uint32_t lo = f16_floor(nc, &fr);
  uint32_t h = f32_bits(nc);  // the murmur3 mix of the four words and its finaliser
  h = rotl32(h * 0xCC9E2D51u, 15) * 0x1B873593u;
  h = rotl32(h ^ (rotl32(f32_bits(g) * 0xCC9E2D51u, 15) * 0x1B873593u), 13) * 5u + 0xE6546B64u;
  h = rotl32(h ^ (rotl32(f32_bits(sg) * 0xCC9E2D51u, 15) * 0x1B873593u), 13) * 5u + 0xE6546B64u;
  h = rotl32(h ^ (rotl32((uint32_t)j * 0xCC9E2D51u, 15) * 0x1B873593u), 13) * 5u + 0xE6546B64u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return lo + (fr > (float)(h >> 19) ? 1u : 0u);
}

}  // namespace dfx
