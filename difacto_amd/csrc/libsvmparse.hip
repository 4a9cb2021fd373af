// libsvm text -> CSR with values on the device.
//
//   dfx_parse_libsvm   ParseLibSVM (difacto_amd/host/reader.cc; the reference's default
//                      data_format, sgd_param.h:57) over a chunk of whole lines already in
//                      device memory
//
// Parallel over bytes and tokens, never one lane per row (the shape of k_tp_tiles / k_tp_cells):
//   k_ls_tiles      every thread takes 16 bytes and marks its separators (' ', '\t', '\n') and
//                   its token ends (a non-separator byte followed by a separator); a tile
//                   (4 KiB) reduces {newlines, tokens, first byte of the open token, tokens
//                   since the last newline}.  This byte pass lives in csrc/linetok.h, which
//                   adfeaparse.hip includes too
//   k_scan_totals   one block scans the tile tuples (csrc/textscan.h: nothing spins)
//   k_ls_finish     rows = newlines, nnz = tokens - rows against the capacities
//   k_ls_cells      the tile's bytes (and the 64 before it) staged in LDS; the same tuple scanned
//                   inside the tile gives every token its line, its number in the line and its
//                   first byte.  The thread owning a token's last byte parses it from LDS: a
//                   line's first token is its label, every other one a feature whose place in
//                   index[] / value[] is (tokens before it) - (rows opened up to and including
//                   its own), so there is no per-line table and no compaction pass.  The thread
//                   owning a '\n' writes offset[row + 1].
// Numbers go through csrc/strtof.h (glibc's strtof bit for bit inside its fast grammar), ids
// through its strtoull (saturating at 2^64 - 1).
//
// The device result is either flagged (stat[2], needs_host) or equal to ParseLibSVM's, never
// silently different.  Parsed on the device: lines  label (blank+ feature)* blank* '\n'  with
// blank = ' ' | '\t', blanks before the label allowed, feature = digits | digits ':' number,
// label and number in the fast grammar, rows with no feature.  The forms that raise the flag,
// and no others:
//   * a label or a value outside the fast grammar of csrc/strtof.h
//   * a feature that is not digits or digits ':' number (an empty id or value, a sign, ...)
//   * a token longer than 64 bytes
//   * a '\r' byte anywhere in the chunk
//   * an empty or blank-only line
//   * a chunk whose last byte is not '\n'
// No byte outside [text, text + nbytes) is read; nothing past max_rows / max_nnz is written.
#include <algorithm>

#include "internal.h"
#include "linetok.h"
#include "strtof.h"

using namespace dfx;

namespace {

constexpr int kLsTokCap = 64;      // the longest token the device parses
constexpr int kLsHalo = kLsTokCap; // bytes staged before the tile: where such a token may begin
constexpr int kLsStage = kLsHalo + kTpTile + 16;

// needs_host bits (kLsCR = 2: the byte pass's, csrc/linetok.h)
constexpr unsigned kLsNumber = 1, kLsEmptyLine = 4, kLsTail = 8, kLsShape = 16, kLsLong = 32;

// stat = {rows, nnz, needs_host (k_ls_flags, after the tokens are parsed), overflow}: every
// line is a row and every token but a line's first a feature
__global__ void k_ls_finish(LsStat* st, const char* text, uint32_t nbytes, int64_t max_rows,
                            int64_t max_nnz, int64_t* stat, uint64_t* offset) {
  if (nbytes && text[nbytes - 1] != '\n') st->flags |= kLsTail;
  const int64_t rows = st->total.nl;
  const int64_t nnz = st->total.tok >= st->total.nl ? st->total.tok - st->total.nl : 0;
  const int over = rows > max_rows || nnz > max_nnz;
  stat[0] = rows;
  stat[1] = nnz;
  stat[2] = 0;
  stat[3] = over;
  if (!over) offset[0] = 0;
}

__global__ void k_ls_flags(const LsStat* st, int64_t* stat) { stat[2] = st->flags != 0; }

__global__ __launch_bounds__(kNT) void k_ls_zero(const int64_t* stat, uint8_t* rowflag) {
  if (stat[3]) return;
  const uint64_t i = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (i < (uint64_t)stat[0]) rowflag[i] = 0;
}

__global__ __launch_bounds__(kNT) void k_ls_cells(const char* text, uint32_t nbytes, int aligned,
                                                  const LsT* tiles, int64_t max_rows,
                                                  int64_t max_nnz, const int64_t* stat,
                                                  uint64_t* offset, uint64_t* index, float* value,
                                                  float* label, uint8_t* rowflag, LsStat* st) {
  __shared__ LsT lds[2 * kNT];
  __shared__ __attribute__((aligned(16))) uint8_t stage[kLsStage];
  if (stat[3]) return;  // overflow: nothing is written
  const uint32_t tile0 = blockIdx.x * kTpTile;
  const uint32_t pos = tile0 + threadIdx.x * kTpBytes;
  const uint4 q = ls_load16(text, nbytes, pos, aligned);
  *reinterpret_cast<uint4*>(stage + kLsHalo + threadIdx.x * kTpBytes) = q;
  if (threadIdx.x < kLsHalo / kTpBytes && tile0 >= (uint32_t)kLsHalo)
    *reinterpret_cast<uint4*>(stage + threadIdx.x * kTpBytes) =
        ls_load16(text, nbytes, tile0 - kLsHalo + threadIdx.x * kTpBytes, aligned);
  if (threadIdx.x == kNT - 1)
    stage[kLsHalo + kTpTile] =
        (uint64_t)tile0 + kTpTile < nbytes ? (uint8_t)text[tile0 + kTpTile] : (uint8_t)'\n';
  __syncthreads();
  const bool next_sep = (uint64_t)pos + kTpBytes >= nbytes ||
                        ls_sep(stage[kLsHalo + (threadIdx.x + 1) * kTpBytes]);
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
    if ((emask >> k) & 1) {  // the token [start, p]
      const uint32_t len = p - start + 1;
      if (len > (uint32_t)kLsTokCap) {
        flags |= kLsLong;
      } else {
        // start >= tile0 - (kLsTokCap - 1): inside the staged bytes
        const LdsGet tok{stage + (kLsHalo + start - tile0)};
        uint32_t bits = 0;
        if (j == 0) {
          if (!dfx_strtof::parse_with(tok, len, &bits)) flags |= kLsNumber;
          if ((int64_t)line < max_rows) label[line] = __uint_as_float(bits);
        } else {
          uint32_t c = 0;
          while (c < len && tok(c) != ':') ++c;
          uint64_t id = 0;
          if (!dfx_strtof::parse_id_with(tok, c, &id)) flags |= kLsShape;
          bits = 0x3f800000u;  // a bare id: 1.0f
          if (c < len && !dfx_strtof::parse_with(LdsGet{tok.s + c + 1}, len - c - 1, &bits))
            flags |= c + 1 == len ? kLsShape : kLsNumber;
          // one label token for every row opened so far; a chunk with an empty line (flagged)
          // may have fewer tokens than that: the difference wraps and fails the bound
          const uint32_t place = tokb - (line + 1);
          if ((int64_t)place < max_nnz && tokb >= line + 1) {
            index[place] = id;
            value[place] = __uint_as_float(bits);
          }
          if (bits != 0x3f800000u && (int64_t)line < max_rows) rowflag[line] = 1;
        }
      }
      ++tokb;
      ++j;
    } else {  // a separator
      start = p + 1;
      if ((nmask >> k) & 1) {
        if (j == 0) flags |= kLsEmptyLine;
        if ((int64_t)line < max_rows)
          offset[(size_t)line + 1] = tokb >= line + 1 ? tokb - (line + 1) : 0;
        ++line;
        j = 0;
      }
    }
  }
  if (flags) atomicOr(&st->flags, flags);
}

}  // namespace

int dfx::parse_libsvm_on(const TpScratch& ws, hipStream_t st, const char* text, int64_t nbytes,
                         int64_t max_rows, int64_t max_nnz, uint64_t* offset, uint64_t* index,
                         float* value, float* label, uint8_t* rowflag, int64_t* stat_dev) {
  DFX_CHECK_ARG(nbytes >= 0 && nbytes < (1ll << 31),
                "parse_libsvm: positions are 32-bit, nbytes must be in [0, 2^31)");
  DFX_CHECK_ARG(max_rows >= 0 && max_nnz >= 0 && offset && stat_dev && (text || nbytes == 0) &&
                    ((label && rowflag) || max_rows == 0) && ((index && value) || max_nnz == 0),
                "parse_libsvm: bad argument");
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
  hipLaunchKernelGGL(k_ls_finish, dim3(1), dim3(1), 0, st, ds, text, (uint32_t)nbytes, max_rows,
                     max_nnz, stat_dev, offset);
  if (nbytes > 0) {
    // a row is at least one byte
    const uint64_t rowcap = (uint64_t)std::min<int64_t>(max_rows, nbytes);
    if (rowcap)
      hipLaunchKernelGGL(k_ls_zero, dim3(blocks_for(rowcap, kNT)), dim3(kNT), 0, st,
                         (const int64_t*)stat_dev, rowflag);
    hipLaunchKernelGGL(k_ls_cells, dim3(ntiles), dim3(kNT), 0, st, text, (uint32_t)nbytes, aligned,
                       (const LsT*)tiles, max_rows, max_nnz, (const int64_t*)stat_dev, offset,
                       index, value, label, rowflag, ds);
  }
  hipLaunchKernelGGL(k_ls_flags, dim3(1), dim3(1), 0, st, (const LsStat*)ds, stat_dev);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

extern "C" int dfx_parse_libsvm(dfx_ctx* ctx, const char* text_dev, int64_t nbytes,
                                int64_t max_rows, int64_t max_nnz, uint64_t* offset,
                                uint64_t* index, float* value, float* label, uint8_t* rowflag,
                                int64_t* stat_dev) {
  DFX_CHECK_ARG(ctx, "null ctx");
  DFX_HIP(hipSetDevice(ctx->c.device));
  Context* c = &ctx->c;
  // the Criteo parser's tile and counter scratch: both run in the input stream's order
  return parse_libsvm_on(context_scratch(c), input_stream(c), text_dev, nbytes, max_rows, max_nnz,
                         offset, index, value, label, rowflag, stat_dev);
}
