// Half-precision V rows (kwarg vrows=f16, V_dim 32 and 64): the pool row is [V: d fp16 | Vaux: d
// fp16] in 4 d bytes, and this is the rounding every write of one goes through.  Integer and exact
// fp32 operations only, the same on the host and the device (vaux16.h's rules: no fp16 type, no
// conversion instruction, no denormal mode): tests/half_ref.py restates them in numpy.
//   read   f16_widen, exact
//   Vaux   vaux16_round, as it stands (vaux16.h)
//   V      vhalf_round below, its signed counterpart
//   InitV, model files, Store.push of a value: f16_nearest
#pragma once
#include "vaux16.h"

namespace dfx {

// The stored fp16 of an updated coordinate nv = v - eta g (adagrad_update), rounded
// stochastically like vaux16_round: the magnitude floors to fp16 (f16_floor), the sign goes back
// on, and the magnitude steps up iff its dropped fraction exceeds r — 13 bits of vaux16_round's
// murmur3 mix over (bits of nv, bits of g, bits of sg, j | 0x10000): g the regularised gradient,
// sg the key's sqrt_g after the UpdateW of the same Update, j the coordinate (the flag keeps V's
// stream apart from Vaux's).  |nv| >= 65504 (or NaN): +-65504.  A value that is an fp16 already
// is stored as it is, so a key whose gradient is zero keeps its V bit for bit.
__host__ __device__ inline uint32_t vhalf_round(float nv, float g, float sg, int j) {
  const uint32_t b = f32_bits(nv), s = (b >> 16) & 0x8000u;
  const float ax = bits_f32(b & 0x7FFFFFFFu);
  if (!(ax < 65504.f)) return s | kF16Max;
  float fr;
  const uint32_t lo = f16_floor(ax, &fr);
  uint32_t h = b;
  h = rotl32(h * 0xCC9E2D51u, 15) * 0x1B873593u;
  h = rotl32(h ^ (rotl32(f32_bits(g) * 0xCC9E2D51u, 15) * 0x1B873593u), 13) * 5u + 0xE6546B64u;
  h = rotl32(h ^ (rotl32(f32_bits(sg) * 0xCC9E2D51u, 15) * 0x1B873593u), 13) * 5u + 0xE6546B64u;
  h = rotl32(h ^ (rotl32(((uint32_t)j | 0x10000u) * 0xCC9E2D51u, 15) * 0x1B873593u), 13) * 5u +
      0xE6546B64u;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return s | (lo + (fr > (float)(h >> 19) ? 1u : 0u));
}

// SGDUpdater::UpdateV for one coordinate of a half row: v and c the widened old values, the
// arithmetic adagrad_update's in fp32 (eta and the new V from the unrounded accumulator); only
// the two results narrow.  -> the stored bits {V, Vaux}
__host__ __device__ inline void vhalf_update(float V_l2, float V_lr, float V_lr_beta, float gV,
                                             float v, float c, float sg, int j, uint32_t* hv,
                                             uint32_t* hc) {
  const float g = gV + V_l2 * v;
  const float nc = sqrtf(c * c + g * g);
  const float eta = V_lr / (nc + V_lr_beta);
  const float nv = v - eta * g;
  *hv = vhalf_round(nv, g, sg, j);
  *hc = vaux16_round(nc, g, sg, j);
}

}  // namespace dfx
