// adfea text -> binary CSR on the device.
//
//   dfx_parse_adfea    ParseAdfea (difacto_amd/host/reader.cc; the reference's CTR format,
//                      src/reader/adfea_parser.h:34-84) over a chunk of whole lines already in
//                      device memory
//
// Parallel over bytes and tokens, never one lane per row; pass 1 is the libsvm parser's byte
// pass (csrc/linetok.h), because inside the domain below a token's role follows from "line
// number, token number in the line":
//   k_ls_tiles      (linetok.h) separators and token ends per 16 bytes, the tuple {newlines,
//                   tokens, first byte of the open token, tokens since the last newline} per tile
//   k_scan_totals   one block scans the tile tuples (csrc/textscan.h: nothing spins)
//   k_ad_finish     rows = newlines, nnz = tokens - 3 * rows against the capacities
//   k_ad_cells      the tile's bytes (and the 64 before it) staged in LDS; the same tuple scanned
//                   inside the tile gives every token its line, its number in the line and its
//                   first byte.  The thread owning a token's last byte parses it from LDS: tokens
//                   0 and 1 of a line (lineid, count) are checked and dropped, token 2 is the
//                   label (1.0f iff its first byte is '1'), every later one a feature idx:gid
//                   -> (idx << 12) | (gid & 4095) whose place in index[] is (tokens before it)
//                   - 3 * (rows opened up to and including its own), so there is no per-line
//                   table and no compaction pass.  The thread owning a '\n' writes
//                   offset[row + 1].  Flags go up by atomicOr: no row flags, nothing to zero.
//   k_ad_flags      stat[2] = a flag was raised
// idx and gid go through csrc/strtof.h's strtoull (saturating at 2^64 - 1); the shift wraps
// mod 2^64 as the host's does.
//
// The device result is either flagged (stat[2], needs_host) or equal to ParseAdfea's, never
// silently different.  Parsed on the device: lines
//   blank* digits blank+ digits blank+ digits (blank+ digits ':' digits)* blank* '\n'
// with blank = ' ' | '\t'.  ParseAdfea's token counter is back at 0 after every such line, so
// its result does not depend on where TextReader::ParseChunk cuts the chunk for its threads.
// The forms that raise the flag, and no others:
//   * an empty or blank-only line, a line with fewer than three tokens
//   * one of a line's first three tokens that is not digits (a "idx:gid" there is the host's
//     row continued on the next line, which the device does not parse)
//   * a later token that is not digits ':' digits
//   * a token longer than 64 bytes
//   * a '\r' byte anywhere in the chunk
//   * a chunk whose last byte is not '\n'
// No byte outside [text, text + nbytes) is read; nothing past max_rows / max_nnz is written.
#include <algorithm>

#include "internal.h"
#include "linetok.h"
#include "strtof.h"

using namespace dfx;

namespace {

constexpr int kAdTokCap = 64;      // the longest token the device parses
constexpr int kAdHalo = kAdTokCap; // bytes staged before the tile: where such a token may begin
constexpr int kAdStage = kAdHalo + kTpTile + 16;
constexpr uint32_t kAdHead = 3;    // lineid, count, label

// needs_host bits (kLsCR = 2: the byte pass's, csrc/linetok.h)
constexpr unsigned kAdHeadShape = 1, kAdShortLine = 4, kAdTail = 8, kAdFeature = 16, kAdLong = 32;

// stat = {rows, nnz, needs_host (k_ad_flags, after the tokens are parsed), overflow}: every
// line is a row and every token but a line's first three a feature.  The tokens of an
// unterminated last line (total.tafter; the chunk is flagged) belong to no row and are not
// counted, so a caller's bound of one feature per ':' holds for such a chunk too.
__global__ void k_ad_finish(LsStat* st, const char* text, uint32_t nbytes, int64_t max_rows,
                            int64_t max_nnz, int64_t* stat, uint64_t* offset) {
  if (nbytes && text[nbytes - 1] != '\n') st->flags |= kAdTail;
  const int64_t rows = st->total.nl;
  const int64_t head = (int64_t)kAdHead * rows;
  const int64_t tok = (int64_t)st->total.tok - (int64_t)st->total.tafter;
  const int64_t nnz = tok >= head ? tok - head : 0;
  const int over = rows > max_rows || nnz > max_nnz;
  stat[0] = rows;
  stat[1] = nnz;
  stat[2] = 0;
  stat[3] = over;
  if (!over) offset[0] = 0;
}

__global__ void k_ad_flags(const LsStat* st, int64_t* stat) { stat[2] = st->flags != 0; }

__global__ __launch_bounds__(kNT) void k_ad_cells(const char* text, uint32_t nbytes, int aligned,
                                                  const LsT* tiles, int64_t max_rows,
                                                  int64_t max_nnz, const int64_t* stat,
                                                  uint64_t* offset, uint64_t* index, float* label,
                                                  LsStat* st) {
  __shared__ LsT lds[2 * kNT];
  __shared__ __attribute__((aligned(16))) uint8_t stage[kAdStage];
  if (stat[3]) return;  // overflow: nothing is written
  const uint32_t tile0 = blockIdx.x * kTpTile;
  const uint32_t pos = tile0 + threadIdx.x * kTpBytes;
  const uint4 q = ls_load16(text, nbytes, pos, aligned);
  *reinterpret_cast<uint4*>(stage + kAdHalo + threadIdx.x * kTpBytes) = q;
  if (threadIdx.x < kAdHalo / kTpBytes && tile0 >= (uint32_t)kAdHalo)
    *reinterpret_cast<uint4*>(stage + threadIdx.x * kTpBytes) =
        ls_load16(text, nbytes, tile0 - kAdHalo + threadIdx.x * kTpBytes, aligned);
  if (threadIdx.x == kNT - 1)
    stage[kAdHalo + kTpTile] =
        (uint64_t)tile0 + kTpTile < nbytes ? (uint8_t)text[tile0 + kTpTile] : (uint8_t)'\n';
  __syncthreads();
  const bool next_sep = (uint64_t)pos + kTpBytes >= nbytes ||
                        ls_sep(stage[kAdHalo + (threadIdx.x + 1) * kTpBytes]);
  uint32_t smask, nmask, emask;
  bool cr;
  ls_masks(q, nbytes, pos, next_sep, &smask, &nmask, &emask, &cr);
  LsT incl, excl, total;
  block_scan<LsOp, kNT>(ls_tuple(pos, smask, nmask, emask), lds, &incl, &excl, &total);
  const LsT in = LsOp::f(tiles[blockIdx.x], excl);
  uint32_t line = in.nl, tokb = in.tok, start = in.last1, j = in.tafter;
  unsigned flags = 0;
  for (uint32_t m = smask | emask; m; m &= m - 1) {
    const int k = __ffs(m) - 1;
    const uint32_t p = pos + k;
    // three head tokens for every row opened so far; a chunk with a short line (flagged) may
    // have fewer tokens than that: no place is then taken from the difference
    const uint64_t head = (uint64_t)kAdHead * ((uint64_t)line + 1);
    if ((emask >> k) & 1) {  // the token [start, p]
      const uint32_t len = p - start + 1;
      if (len > (uint32_t)kAdTokCap) {
        flags |= kAdLong;
      } else {
        // start >= tile0 - (kAdTokCap - 1): inside the staged bytes
        const LdsGet tok{stage + (kAdHalo + start - tile0)};
        uint64_t idx = 0, gid = 0;
        if (j < kAdHead) {
          if (!dfx_strtof::parse_id_with(tok, len, &idx)) flags |= kAdHeadShape;
          if (j == kAdHead - 1 && (int64_t)line < max_rows) label[line] = tok(0) == '1' ? 1.f : 0.f;
        } else {
          uint32_t c = 0;
          while (c < len && tok(c) != ':') ++c;
          if (c == len || !dfx_strtof::parse_id_with(tok, c, &idx) ||
              !dfx_strtof::parse_id_with(LdsGet{tok.s + c + 1}, len - c - 1, &gid))
            flags |= kAdFeature;
          const uint64_t place = (uint64_t)tokb - head;
          if ((uint64_t)tokb >= head && (int64_t)place < max_nnz)
            index[place] = (idx << 12) | (gid & 4095u);
        }
      }
      ++tokb;
      ++j;
    } else {  // a separator
      start = p + 1;
      if ((nmask >> k) & 1) {
        if (j < kAdHead) flags |= kAdShortLine;
        if ((int64_t)line < max_rows)
          offset[(size_t)line + 1] = (uint64_t)tokb >= head ? (uint64_t)tokb - head : 0;
        ++line;
        j = 0;
      }
    }
  }
  if (flags) atomicOr(&st->flags, flags);
}

}  // namespace

int dfx::parse_adfea_on(const TpScratch& ws, hipStream_t st, const char* text, int64_t nbytes,
                        int64_t max_rows, int64_t max_nnz, uint64_t* offset, uint64_t* index,
                        float* label, int64_t* stat_dev) {
  DFX_CHECK_ARG(nbytes >= 0 && nbytes < (1ll << 31),
                "parse_adfea: positions are 32-bit, nbytes must be in [0, 2^31)");
  DFX_CHECK_ARG(max_rows >= 0 && max_nnz >= 0 && offset && stat_dev && (text || nbytes == 0) &&
                    (label || max_rows == 0) && (index || max_nnz == 0),
                "parse_adfea: bad argument");
  const uint32_t ntiles = blocks_for((uint64_t)nbytes, kTpTile);
  DFX_TRY(ws.tiles->ensure((size_t)std::max(ntiles, 1u) * sizeof(LsT)));
  DFX_TRY(ws.stat->ensure(sizeof(LsStat)));
  LsT* tiles = ws.tiles->as<LsT>();
  LsStat* ds = ws.stat->as<LsStat>();
  const int aligned = (reinterpret_cast<uintptr_t>(text) & 15) == 0;
  DFX_HIP(hipMemsetAsync(ds, 0, sizeof(LsStat), st));
  if (nbytes > 0) {
    hipLaunchKernelGGL(k_ls_tiles, dim3(ntiles), dim3(kNT), 0, st, text, (uint32_t)nbytes, aligned,
                       tiles, ds);
    hipLaunchKernelGGL((k_scan_totals<LsOp>), dim3(1), dim3(1024), 0, st, tiles,
                       (const uint32_t*)nullptr, (uint32_t)nbytes, (uint32_t)kTpTile, &ds->total);
  }
  hipLaunchKernelGGL(k_ad_finish, dim3(1), dim3(1), 0, st, ds, text, (uint32_t)nbytes, max_rows,
                     max_nnz, stat_dev, offset);
  if (nbytes > 0)
    hipLaunchKernelGGL(k_ad_cells, dim3(ntiles), dim3(kNT), 0, st, text, (uint32_t)nbytes, aligned,
                       (const LsT*)tiles, max_rows, max_nnz, (const int64_t*)stat_dev, offset,
                       index, label, ds);
  hipLaunchKernelGGL(k_ad_flags, dim3(1), dim3(1), 0, st, (const LsStat*)ds, stat_dev);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

extern "C" int dfx_parse_adfea(dfx_ctx* ctx, const char* text_dev, int64_t nbytes,
                               int64_t max_rows, int64_t max_nnz, uint64_t* offset,
                               uint64_t* index, float* label, int64_t* stat_dev) {
  DFX_CHECK_ARG(ctx, "null ctx");
  DFX_HIP(hipSetDevice(ctx->c.device));
  Context* c = &ctx->c;
  // the Criteo parser's tile and counter scratch: all three run in the input stream's order
  return parse_adfea_on(context_scratch(c), input_stream(c), text_dev, nbytes, max_rows, max_nnz,
                        offset, index, label, stat_dev);
}
