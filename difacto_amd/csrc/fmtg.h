// A prediction row as text, exactly as the driver's host loop prints it
// (SGDLearner::SavePred, sgd_learner.h:72-83):
//
//   fprintf(f, "%g\t%g\n", label, pred_prob ? 1.0 / (1.0 + std::exp(-pred)) : (double)pred);
//
// One text for the host (tools/fmtg_check.cc, g++) and the device (csrc/predtext.hip, hipcc);
// integer arithmetic only once the double is formed.  An answer is glibc's bytes or "needs
// host" (a negative length), never silently different.
//
// %g at the default precision 6 of a finite x != 0: let X be the decimal exponent of x after it
// is rounded to six significant digits (round half to even on the exact binary value).  The
// digits d0..d5 print as d0.d1d2d3d4d5e[+-]XX when X < -4 or X >= 6 (at least two exponent
// digits), else in %f form with 5 - X decimals; trailing zeros of the fraction and a bare point
// are dropped either way.  Zeros print as 0 and -0.
//
// The conversion: x = m * 2^e with m < 2^53.  With k = 5 - X, the six digits are
// round(m * 2^e * 10^k).
//   k >= 0 (k <= 19): m * 10^k < 2^53 * 2^64 is one 64x64 -> 128-bit product in two words; the
//                     digits are its bits above bit -e, the bits below against half decide the
//                     rounding (e < 0, -e <= 120)
//   k <  0 (k >= -6): m / (10^-k * 2^-e) with the divisor below 2^63, the remainder against
//                     half of it
// X starts from floor(log2 x) and is corrected by the digits themselves (at most two steps), a
// carry out of 999999.5 moves it once more.  That covers 1e-14 <= |x| < 1e12; the guaranteed
// domain, +-0 and 1e-12 <= |x| < 1e12, lies inside it.  Non-finite values, subnormals and
// anything outside need the host.  In the guaranteed domain a field has at most 12 bytes
// (-d.ddddde-XX, -0.000dddddd), a row "label\tvalue\n" at most 26.
#pragma once
#include <stdint.h>

#include "expf.h"

#if defined(__HIPCC__)
#define DFX_FMTG_HD __host__ __device__ inline
#else
#define DFX_FMTG_HD inline
#endif

namespace dfx_fmtg {

constexpr int kRecBytes = 32;   // a row's record: its text, zero filled; byte 31 holds the length
constexpr int kMaxField = 12;   // bytes of one %g field
constexpr int kMaxRow = 2 * kMaxField + 2;

DFX_FMTG_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// 10^k, 0 <= k <= 19
DFX_FMTG_HD uint64_t pow10_u64(int k) {
  uint64_t p = 1;
  for (int i = 0; i < 19; ++i) p *= i < k ? 10u : 1u;
  return p;
}

// floor(m * 2^e * 10^k) -> *q, and the rest against one half (-1 below, 0 a tie, 1 above) ->
// *cmp; false where the two words do not hold it
DFX_FMTG_HD bool scaled(uint64_t m, int e, int k, uint64_t* q, int* cmp) {
  if (e >= 0) return false;
  const int s = -e;
  if (k >= 0) {
    if (k > 19 || s > 120) return false;
    const uint64_t p = pow10_u64(k);
    const uint64_t lo = m * p, hi = mulhi64(m, p);
    uint64_t rh, rl, hh, hl;  // the rest and one half, two words each
    if (s < 64) {
      if (hi >> s) return false;
      *q = (hi << (64 - s)) | (lo >> s);
      rh = 0;
      rl = lo & ((1ull << s) - 1);
      hh = 0;
      hl = 1ull << (s - 1);
    } else if (s == 64) {
      *q = hi;
      rh = 0;
      rl = lo;
      hh = 0;
      hl = 1ull << 63;
    } else {
      *q = hi >> (s - 64);
      rh = hi & ((1ull << (s - 64)) - 1);
      rl = lo;
      hh = 1ull << (s - 65);
      hl = 0;
    }
    *cmp = rh != hh ? (rh < hh ? -1 : 1) : rl != hl ? (rl < hl ? -1 : 1) : 0;
    return true;
  }
  if (k < -6 || s > 43) return false;
  const uint64_t d = pow10_u64(-k) << s;  // < 2^20 * 2^43
  *q = m / d;
  const uint64_t r2 = (m % d) * 2;
  *cmp = r2 != d ? (r2 < d ? -1 : 1) : 0;
  return true;
}

// snprintf(out, ., "%g", x) without the terminator -> the length (<= kMaxField), or -1: needs
// the host (nothing of out is to be used)
DFX_FMTG_HD int fmt_g(double x, char* out) {
  uint64_t b = __builtin_bit_cast(uint64_t, x);
  int n = 0;
  if (b >> 63) out[n++] = '-';
  b &= ~(1ull << 63);
  if (b == 0) {
    out[n++] = '0';
    return n;
  }
  const int be = (int)(b >> 52);
  if (be == 0 || be == 0x7ff) return -1;  // subnormal, inf, nan
  const uint64_t m = (b & ((1ull << 52) - 1)) | (1ull << 52);
  const int e = be - 1075;                    // x = m * 2^e
  int X = ((be - 1023) * 78913) >> 18;        // floor(floor(log2 x) * log10 2): X or X - 1
  uint64_t q = 0;
  int cmp = 0;
  bool ok = false;
  for (int t = 0; t < 3 && !ok; ++t) {
    if (!scaled(m, e, 5 - X, &q, &cmp)) return -1;
    if (q >= 1000000u) ++X;
    else if (q < 100000u) --X;
    else ok = true;
  }
  if (!ok) return -1;
  if (cmp > 0 || (cmp == 0 && (q & 1u))) ++q;
  if (q == 1000000u) {
    q = 100000u;
    ++X;
  }
  if (X < -14 || X > 12) return -1;  // (12: the carry out of 999999.5e6)
  char d[6];
  uint32_t r = (uint32_t)q;
  for (int i = 5; i >= 0; --i) {
    d[i] = (char)('0' + r % 10u);
    r /= 10u;
  }
  int nd = 6;
  while (nd > 1 && d[nd - 1] == '0') --nd;
  if (X < -4 || X >= 6) {
    out[n++] = d[0];
    if (nd > 1) out[n++] = '.';
    for (int i = 1; i < 6; ++i)
      if (i < nd) out[n++] = d[i];
    out[n++] = 'e';
    out[n++] = X < 0 ? '-' : '+';
    const int ax = X < 0 ? -X : X;  // <= 14
    out[n++] = (char)('0' + ax / 10);
    out[n++] = (char)('0' + ax % 10);
  } else if (X >= 0) {
    for (int i = 0; i < 6; ++i)
      if (i <= X) out[n++] = d[i];
    if (nd > X + 1) out[n++] = '.';
    for (int i = 1; i < 6; ++i)
      if (i > X && i < nd) out[n++] = d[i];
  } else {
    out[n++] = '0';
    out[n++] = '.';
    for (int i = 1; i < 4; ++i)
      if (i < -X) out[n++] = '0';
    for (int i = 0; i < 6; ++i)
      if (i < nd) out[n++] = d[i];
  }
  return n;
}

// the value a row prints: the probability as the host loop forms it (std::exp on a float is
// expf, the add and the divide are IEEE doubles), or the raw prediction
template <typename Tab>
DFX_FMTG_HD double pred_value(float pred, int pred_prob, const Tab& tab) {
  return pred_prob ? 1.0 / (1.0 + (double)dfx::expf_glibc(-pred, tab)) : (double)pred;
}

// "label\tvalue\n" into rec[0 .. kRecBytes) -> its length (<= kMaxRow), or -1: needs the host.
// Bytes past the length are whatever rec held.
DFX_FMTG_HD int fmt_row(float label, double value, char* rec) {
  const int a = fmt_g((double)label, rec);
  if (a < 0) return -1;
  rec[a] = '\t';
  const int b = fmt_g(value, rec + a + 1);
  if (b < 0) return -1;
  rec[a + 1 + b] = '\n';
  return a + b + 2;
}

}  // namespace dfx_fmtg
