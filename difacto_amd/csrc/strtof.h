// Decimal text -> float bits, exactly as glibc's strtof rounds it, for the tokens a libsvm file
// is made of.  One text for the host (tools/strtof_check.cc, g++) and the device parser
// (csrc/libsvmparse.hip, hipcc); integer arithmetic only.
//
// The fast grammar, which a token must match in full:
//
//   [+-]? ( digits ( '.' digits? )? | '.' digits ) ( [eE] [+-]? digits{1,3} )?
//
// with at most 19 digits after the leading zeros are stripped (trailing zeros count), so the
// number is w * 10^q, w < 10^19 < 2^64, q = exponent - fraction digits.
//   w == 0      -> +-0, whatever q is
//   |q| <= 27   -> the correctly rounded float (round half to even), or +-inf past FLT_MAX:
//                  q >= 0: w * 5^q is one 64x64 -> 128-bit product (5^27 < 2^63)
//                  q <  0: w / 5^-q by a shift-subtract division of the normalised operands,
//                          27 quotient bits, the remainder's "non-zero" as the sticky bit
//                  then one round-to-nearest-even to 24 bits.  w * 10^q >= 10^-27 is never
//                  subnormal; overflow needs q >= 20 and is a comparison of the exponent.
// Everything else is "not fast" (return false), never guessed: more digits, a larger |q|, hex
// floats, inf / nan, "1e", "1.5abc", an empty string.
//
// dfx_strtof::parse_id is strtoull(base 10) on a run of digits: saturating at 2^64 - 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFX_STRTOF_HD __host__ __device__ inline
#else
#define DFX_STRTOF_HD inline
#endif

namespace dfx_strtof {

constexpr int kMaxDigits = 19;  // significant digits of the fast grammar
constexpr int kMaxQ = 27;       // |q| of the fast grammar: 5^27 < 2^63

DFX_STRTOF_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

DFX_STRTOF_HD int clz64(uint64_t x) { return __builtin_clzll(x); }  // x != 0

// (hi:lo, sticky) * 2^e, hi:lo != 0, rounded half to even to a float's 24 bits
DFX_STRTOF_HD uint32_t round_bits(uint64_t hi, uint64_t lo, bool sticky, int e, uint32_t sign) {
  const int len = hi ? 128 - clz64(hi) : 64 - clz64(lo);  // bit length
  int shift = len - 24;
  uint32_t m;
  if (shift <= 0) {
    m = (uint32_t)lo << -shift;  // exact
  } else {
    // the 24 bits from bit `shift` up, the round bit below them, the rest ORed into sticky
    uint64_t top, rest;  // top: bits [shift - 1, shift + 24), rest: non-zero iff bits below
    const int s1 = shift - 1;
    if (s1 == 0) {
      top = lo;
      rest = 0;
    } else if (s1 < 64) {
      top = (lo >> s1) | (hi << (64 - s1));
      rest = lo << (64 - s1);
    } else if (s1 == 64) {
      top = hi;
      rest = lo;
    } else {
      top = hi >> (s1 - 64);
      rest = (hi << (128 - s1)) | lo;
    }
    const uint32_t t = (uint32_t)top & 0x1ffffffu;  // 25 bits
    m = t >> 1;
    const bool half = t & 1u, low = sticky || rest != 0;
    if (half && (low || (m & 1u))) ++m;
    if (m == (1u << 24)) {
      m >>= 1;
      ++shift;
    }
  }
  const int ex = shift + e + 23;  // the unbiased exponent of the leading bit
  if (ex > 127) return sign | 0x7f800000u;
  return sign | ((uint32_t)(ex + 127) << 23) | (m & 0x7fffffu);
}

// w * 10^q, w != 0, |q| <= kMaxQ
DFX_STRTOF_HD uint32_t scale_bits(uint64_t w, int q, uint32_t sign) {
  uint64_t p5 = 1;
  const int k = q < 0 ? -q : q;
  for (int i = 0; i < k; ++i) p5 *= 5;
  if (q >= 0) return round_bits(mulhi64(w, p5), w * p5, false, q, sign);
  // w / 5^k * 2^-k: both operands with their top bit set, 27 quotient bits by shift-subtract
  const int cw = clz64(w), cd = clz64(p5);
  const uint64_t d = p5 << cd;
  uint64_t r = w << cw, quo = 0;
  for (int i = 0; i < 27; ++i) {
    bool bit;
    if (i == 0) {
      bit = r >= d;
    } else {
      const bool carry = r >> 63;
      r <<= 1;
      bit = carry || r >= d;
    }
    if (bit) r -= d;  // modulo 2^64 with the carry: the true remainder
    quo = (quo << 1) | (uint64_t)bit;
  }
  // w / 5^k = quo * 2^(-26 + cd - cw) and a remainder
  return round_bits(0, quo, r != 0, cd - cw - k - 26, sign);
}

// the token s[0, len) -> *bits; false: not in the fast grammar.  Get(i) reads byte i.
template <class Get>
DFX_STRTOF_HD bool parse_with(Get get, uint32_t len, uint32_t* bits) {
  uint32_t i = 0;
  uint32_t sign = 0;
  if (i < len && (get(i) == '+' || get(i) == '-')) {
    sign = get(i) == '-' ? 0x80000000u : 0u;
    ++i;
  }
  uint64_t w = 0;
  int nsig = 0, nfrac = 0, ndig = 0;
  bool point = false;
  for (; i < len; ++i) {
    const uint32_t c = (uint8_t)get(i);
    if (c == '.') {
      if (point) return false;
      point = true;
      continue;
    }
    const uint32_t dg = c - (uint32_t)'0';
    if (dg > 9) break;
    ++ndig;
    if (point) ++nfrac;
    if (nsig || dg) {
      if (++nsig > kMaxDigits) return false;
      w = w * 10 + dg;
    }
  }
  if (ndig == 0) return false;
  int ex = 0;
  if (i < len) {
    if (get(i) != 'e' && get(i) != 'E') return false;
    ++i;
    bool eneg = false;
    if (i < len && (get(i) == '+' || get(i) == '-')) {
      eneg = get(i) == '-';
      ++i;
    }
    const uint32_t nexp = len - i;
    if (nexp < 1 || nexp > 3) return false;
    for (; i < len; ++i) {
      const uint32_t dg = (uint32_t)(uint8_t)get(i) - (uint32_t)'0';
      if (dg > 9) return false;
      ex = ex * 10 + (int)dg;
    }
    if (eneg) ex = -ex;
  }
  if (w == 0) {
    *bits = sign;
    return true;
  }
  const int q = ex - nfrac;
  if (q > kMaxQ || q < -kMaxQ) return false;
  *bits = scale_bits(w, q, sign);
  return true;
}

struct PtrGet {
  const char* s;
  DFX_STRTOF_HD char operator()(uint32_t i) const { return s[i]; }
};

DFX_STRTOF_HD bool parse(const char* s, uint32_t len, uint32_t* bits) {
  return parse_with(PtrGet{s}, len, bits);
}

// strtoull(base 10) on the digits s[0, n): false when a byte is not a digit or n == 0
template <class Get>
DFX_STRTOF_HD bool parse_id_with(Get get, uint32_t n, uint64_t* out) {
  if (n == 0) return false;
  uint64_t v = 0;
  bool sat = false;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t dg = (uint32_t)(uint8_t)get(i) - (uint32_t)'0';
    if (dg > 9) return false;
    // v * 10 + dg > 2^64 - 1
    if (v > 0x1999999999999999ull || (v == 0x1999999999999999ull && dg > 5)) sat = true;
    v = v * 10 + dg;
  }
  *out = sat ? ~0ull : v;
  return true;
}

DFX_STRTOF_HD bool parse_id(const char* s, uint32_t n, uint64_t* out) {
  return parse_id_with(PtrGet{s}, n, out);
}

}  // namespace dfx_strtof
