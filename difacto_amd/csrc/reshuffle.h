// The per-epoch row permutation of the device reshuffler (reshuffle.hip): a keyed bijection on
// [0, N) computed independently per row, with no permutation array, no sort and no host list.
// Plain C++ (no HIP types): the device kernels, tools/reshuffle_check.cc and the numpy
// restatement tests/reshuffle_ref.py all read THIS text; change them together.
//
// Family: a balanced Feistel network over b bits with cycle walking.
//   b     the least EVEN number of bits with 2^b >= N, at least 2, so 2^b < 4 N for N >= 2
//         (N <= 1: the identity, nothing is walked)
//   split equal halves of h = b / 2 bits, x = L << h | R
//   round (L, R) -> (R, L ^ (rs_fmix32(R ^ k[r]) & (2^h - 1))), r = 0 .. kRsRounds - 1
//   keys  k[r] = the low 32 bits of the r-th output of splitmix64 seeded with `key`
//   walk  the network is applied again to its own output until the value is below N (a cycle of
//         a bijection of [0, 2^b) restricted to [0, N) is again a bijection); fewer than 4 tries
//         in the mean, a per-row loop
// rs_fmix32 is MurmurHash3's 32-bit finalizer, rs_splitmix64 the splitmix64 generator's step.
//
// Seed: rs_epoch_key(shuffle_seed, epoch, list) chains three splitmix64 steps:
//   a = splitmix64(shuffle_seed), b = splitmix64(a ^ epoch), key = splitmix64(b ^ list).
//
// The per-epoch negative down-sample (dfx_reshuffle_begin_epoch_sampled): a keyed draw per row
// beside the keyed position, read by the kernels, tools/resample_check.cc and the numpy
// restatement tests/resample_ref.py.
//   rs_draw(key, row)  u in [0, 1), a multiple of 2^-24 (exact in fp32): the top 24 bits of one
//                      splitmix64 output of the state key ^ (0xA0761D6478BD642F * (row + 1))
//   rs_dropped         the reader's own inequality (host/reader.cc, restating the reference's
//                      batch_reader.cc:57-63), in fp32, its rand_r draw p replaced by u: a row
//                      with label <= 0 is dropped when u > 1 - neg_sampling.  That drops a
//                      negative with probability neg_sampling (the reference does the same,
//                      whatever the parameter's doc comment says: the contract is its behaviour);
//                      a positive row is never dropped, and neg_sampling >= 1 drops nothing: the
//                      reader draws only when neg_sampling < 1 (reader.cc:817), and so does
//                      this (without that guard u > 1 - 1 would drop every row but u = 0).
//   row   the SOURCE row: its position in the concatenation of the list's batches, not the
//         position the permutation gives it in the output
//   key   the epoch key the permutation of that epoch uses (rs_epoch_key)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__
#else
#define RS_HD
#endif

constexpr int kRsRounds = 4;

// one step of splitmix64: advances *state, returns the output
RS_HD inline uint64_t rs_splitmix64(uint64_t* state) {
  *state += 0x9E3779B97F4A7C15ull;
  uint64_t z = *state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

RS_HD inline uint32_t rs_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// the network of one (N, key): by value into a kernel
struct rs_net {
  uint32_t k[kRsRounds];
  uint32_t n;     // N
  uint32_t half;  // h = b / 2 (0: N <= 1)
};

RS_HD inline rs_net rs_make(uint32_t N, uint64_t key) {
  rs_net t;
  uint64_t s = key;
  for (int r = 0; r < kRsRounds; ++r) t.k[r] = (uint32_t)rs_splitmix64(&s);
  t.n = N;
  uint32_t b = 0;
  if (N > 1) {
    b = 2;
    while (b < 32 && (1ull << b) < (uint64_t)N) b += 2;
  }
  t.half = b / 2;
  return t;
}

RS_HD inline uint32_t rs_apply(const rs_net& t, uint32_t j) {
  if (t.half == 0) return j;
  const uint32_t h = t.half, m = (1u << h) - 1u;
  uint32_t x = j;
  do {
    uint32_t L = x >> h, R = x & m;
    for (int r = 0; r < kRsRounds; ++r) {
      const uint32_t f = rs_fmix32(R ^ t.k[r]) & m;
      const uint32_t nl = R;
      R = L ^ f;
      L = nl;
    }
    x = L << h | R;
  } while (x >= t.n);
  return x;
}

// position j of the output takes row rs_perm(j, N, key) of the input; N < 2^31
RS_HD inline uint32_t rs_perm(uint32_t j, uint32_t N, uint64_t key) {
  return rs_apply(rs_make(N, key), j);
}

// u in [0, 1), a multiple of 2^-24, exact in fp32
RS_HD inline float rs_draw(uint64_t key, uint32_t row) {
  uint64_t s = key ^ (0xA0761D6478BD642Full * ((uint64_t)row + 1));
  return (float)(rs_splitmix64(&s) >> 40) * (1.f / 16777216.f);  // 2^-24 (host code is C++14)
}

// the reader's own inequality (reader.cc:817-820), p replaced by the keyed draw
RS_HD inline bool rs_dropped(uint64_t key, uint32_t row, float label, float neg_sampling) {
  return neg_sampling < 1.f && label <= 0.f && rs_draw(key, row) > 1.f - neg_sampling;
}

RS_HD inline uint64_t rs_epoch_key(uint64_t shuffle_seed, uint64_t epoch, uint64_t list) {
  uint64_t s = shuffle_seed;
  const uint64_t a = rs_splitmix64(&s);
  s = a ^ epoch;
  const uint64_t b = rs_splitmix64(&s);
  s = b ^ list;
  return rs_splitmix64(&s);
}
