// A model entry as the two model files hold it, exactly as the host writers lay it down
// (csrc/store.hip dfx_store_save / dfx_store_dump, which restate SGDUpdater::Save and ::Dump,
// src/sgd/sgd_updater.h:84-139 with SGDEntry::SaveEntry :35-48):
//
//   binary  key(8) int size(4) w(4) [sqrt_g(4) z(4)] [V(4 d)] [Vaux(4 d)]
//   text    key \t size \t w [\t sqrt_g \t z] [\t V..] [\t Vaux..] \n
//
// with size = 1 + d for an entry that has V and 1 for one that has none, the bracketed state
// and Vaux under save_aux / dump_aux only, and an entry with w == 0.f and no V left out of both
// (SGDEntry::empty(); a float compare, so -0.f counts).  The text prints the key as a decimal
// (after reverse_bytes under need_reverse), size as a decimal and every float as `ostream <<
// float` does: %g at precision 6 of the float widened to double, which is csrc/fmtg.h's fmt_g.
//
// One text for the host (tools/modeltext_check.cc, g++, against a real std::ostream) and the
// device (csrc/modelfile.hip).  A line is a sequence of fields, each followed by its separator
// ('\t', or '\n' behind the last), so a file's text is the concatenation of its fields in slot
// and field order: the device formats a field per lane.  An answer is the host's bytes or "needs
// host" (a negative length: a float outside fmt_g's domain), never silently different.
#pragma once
#include <stdint.h>

#include "fmtg.h"
#include "revbytes.h"

namespace dfx_modeltext {

constexpr int kMaxKey = 20;                       // 2^64 - 1 has 20 digits
constexpr int kMaxFloat = dfx_fmtg::kMaxField;    // 12
constexpr int kFieldBytes = 24;                   // room for any field and its separator

// the decimal of v -> its length (1..20)
DFX_FMTG_HD int fmt_u64(uint64_t v, char* out) {
  int n = 1;
  for (uint64_t t = v; t >= 10u; t /= 10u) ++n;
  for (int i = n - 1; i >= 0; --i) {
    out[i] = (char)('0' + (int)(v % 10u));
    v /= 10u;
  }
  return n;
}

// the key a line prints
DFX_FMTG_HD uint64_t printed_key(uint64_t key, int need_reverse) {
  return need_reverse ? dfx::reverse_bytes(key) : key;
}

// an entry that neither file holds
DFX_FMTG_HD bool entry_empty(float w, bool has_v) { return w == 0.f && !has_v; }

// bytes of a binary record
DFX_FMTG_HD int record_bytes(bool has_v, int d, int aux) {
  return 16 + (aux ? 8 : 0) + (has_v ? 4 * d * (aux ? 2 : 1) : 0);
}
// dwords of a record in front of its V row: key, size, w [, sqrt_g, z]
DFX_FMTG_HD int record_head_dwords(int aux) { return aux ? 6 : 4; }

// fields of a text line
DFX_FMTG_HD int line_fields(bool has_v, int d, int aux) {
  return 3 + (aux ? 2 : 0) + (has_v ? d * (aux ? 2 : 1) : 0);
}
// bytes of the longest line whose floats are all inside fmt_g's domain
DFX_FMTG_HD int64_t worst_line_bytes(int d, int aux) {
  return (kMaxKey + 1) + (10 + 1) + (int64_t)(kMaxFloat + 1) * (line_fields(true, d, aux) - 2);
}

// what field j of a line holds; *k: the coordinate of a V / Vaux field
enum Field { kKey, kSize, kW, kSqrtG, kZ, kV, kVaux };
DFX_FMTG_HD Field field_of(int j, int d, int aux, int* k) {
  *k = 0;
  if (j == 0) return kKey;
  if (j == 1) return kSize;
  if (j == 2) return kW;
  int r = j - 3;
  if (aux) {
    if (r == 0) return kSqrtG;
    if (r == 1) return kZ;
    r -= 2;
  }
  if (r < d) {
    *k = r;
    return kV;
  }
  *k = r - d;
  return kVaux;
}

// one field and its separator into out[0 .. kFieldBytes) -> the bytes (<= 21), or -1: needs
// the host.  u: the printed key or the size of an integer field; f: the float of any other
DFX_FMTG_HD int fmt_field(Field what, uint64_t u, float f, bool last, char* out) {
  const int n = what == kKey || what == kSize ? fmt_u64(u, out) : dfx_fmtg::fmt_g((double)f, out);
  if (n < 0) return -1;
  out[n] = last ? '\n' : '\t';
  return n + 1;
}

// a whole line by one caller (the host tool; the device goes field by field) into out, which
// holds worst_line_bytes(d, aux) -> its length, or -1: needs the host.  V, C: the entry's rows
// (null without V); key: as stored
DFX_FMTG_HD int64_t fmt_line(uint64_t key, int need_reverse, float w, float sqrt_g, float z,
                             const float* V, const float* C, int d, int aux, char* out) {
  const int nf = line_fields(V != nullptr, d, aux);
  int64_t n = 0;
  for (int j = 0; j < nf; ++j) {
    int k;
    const Field what = field_of(j, d, aux, &k);
    const uint64_t u = what == kKey ? printed_key(key, need_reverse) : (uint64_t)(V ? 1 + d : 1);
    const float f = what == kW ? w : what == kSqrtG ? sqrt_g : what == kZ ? z
                    : what == kV ? V[k] : what == kVaux ? C[k] : 0.f;
    char buf[kFieldBytes];
    const int L = fmt_field(what, u, f, j == nf - 1, buf);
    if (L < 0) return -1;
    for (int i = 0; i < L; ++i) out[n + i] = buf[i];
    n += L;
  }
  return n;
}

}  // namespace dfx_modeltext
