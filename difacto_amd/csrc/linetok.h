// The byte pass of the line-and-token text parsers (libsvmparse.hip: libsvm; adfeaparse.hip:
// adfea): lines end at '\n', tokens are separated by ' ' | '\t' | '\n', and what a token means
// follows from "line number, token number in the line".  Every thread takes 16 bytes and marks
// its separators and its token ends (a non-separator byte followed by a separator); the tuple
// {newlines, tokens, first byte of the open token, tokens since the last newline} is reduced per
// 4 KiB tile here (k_ls_tiles), scanned over the tiles by k_scan_totals<LsOp> (textscan.h) and
// scanned again inside a tile by the format's token kernel.  As textscan.h's helpers these sit
// in an unnamed namespace: each .hip file that includes them gets kernels of its own.
#pragma once
#include "textscan.h"

namespace {

// needs_host bit of a '\r' byte anywhere in the chunk: the byte pass raises it for both formats
constexpr unsigned kLsCR = 2;

// {newlines, token ends, 1 + position of the last separator (= first byte of the open token;
// 0: none), token ends since the last newline}; combining is associative, left to right
struct LsT {
  uint32_t nl, tok, last1, tafter;
};
struct LsOp {
  using T = LsT;
  __device__ static T id() { return LsT{0, 0, 0, 0}; }
  __device__ static T f(const T& a, const T& b) {
    return LsT{a.nl + b.nl, a.tok + b.tok, b.last1 ? b.last1 : a.last1,
               b.nl ? b.tafter : a.tafter + b.tafter};
  }
};

struct LsStat {
  unsigned int flags;  // the format's needs_host bits
  LsT total;           // the byte pass's grand total
};

__device__ inline bool ls_sep(uint32_t c) { return c == ' ' || c == '\t' || c == '\n'; }

// the 16 bytes at pos; bytes at or past nbytes read as 0
__device__ inline uint4 ls_load16(const char* text, uint32_t nbytes, uint32_t pos, int aligned) {
  if (aligned && (uint64_t)pos + kTpBytes <= nbytes)
    return *reinterpret_cast<const uint4*>(text + pos);
  uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < kTpBytes; ++k)
    if ((uint64_t)pos + k < nbytes)
      w[k >> 2] |= (uint32_t)(uint8_t)text[pos + k] << (8 * (k & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// masks of the separators / newlines / token ends among the 16 bytes q at pos; next_sep: the
// byte at pos + 16 is a separator or past the text.  Bytes past the text are no tokens.
__device__ inline void ls_masks(const uint4& q, uint32_t nbytes, uint32_t pos, bool next_sep,
                                uint32_t* smask, uint32_t* nmask, uint32_t* emask, bool* cr) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  const uint32_t nvalid = pos >= nbytes ? 0u : (nbytes - pos < 16u ? nbytes - pos : 16u);
  const uint32_t v = (1u << nvalid) - 1u;
  uint32_t s = 0, n = 0, r = 0;
#pragma unroll
  for (int k = 0; k < kTpBytes; ++k) {
    const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 255u;
    s |= (uint32_t)ls_sep(c) << k;
    n |= (uint32_t)(c == '\n') << k;
    r |= (uint32_t)(c == '\r') << k;
  }
  s &= v, n &= v, r &= v;
  const uint32_t ext = s | (~v & 0xffffu) | ((uint32_t)next_sep << 16);
  *smask = s;
  *nmask = n;
  *emask = (v & ~s) & (ext >> 1);
  *cr = r != 0;
}

__device__ inline LsT ls_tuple(uint32_t pos, uint32_t smask, uint32_t nmask, uint32_t emask) {
  LsT t;
  t.nl = __popc(nmask);
  t.tok = __popc(emask);
  t.last1 = smask ? pos + (31 - __clz(smask)) + 1 : 0;
  t.tafter = nmask ? __popc(emask >> (32 - __clz(nmask))) : __popc(emask);
  return t;
}

__global__ __launch_bounds__(kNT) void k_ls_tiles(const char* text, uint32_t nbytes, int aligned,
                                                  LsT* tiles, LsStat* st) {
  __shared__ LsT lds[2 * kNT];
  const uint32_t pos = blockIdx.x * kTpTile + threadIdx.x * kTpBytes;
  const uint4 q = ls_load16(text, nbytes, pos, aligned);
  const bool next_sep =
      (uint64_t)pos + kTpBytes >= nbytes || ls_sep((uint8_t)text[pos + kTpBytes]);
  uint32_t smask, nmask, emask;
  bool cr;
  ls_masks(q, nbytes, pos, next_sep, &smask, &nmask, &emask, &cr);
  if (cr) atomicOr(&st->flags, kLsCR);
  LsT incl, excl, total;
  block_scan<LsOp, kNT>(ls_tuple(pos, smask, nmask, emask), lds, &incl, &excl, &total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

// a token's bytes in a token kernel's LDS stage, for dfx_strtof's parsers
struct LdsGet {
  const uint8_t* s;
  __device__ char operator()(uint32_t i) const { return (char)s[i]; }
};

}  // namespace
