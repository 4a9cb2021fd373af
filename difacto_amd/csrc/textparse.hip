// Criteo text -> CSR on the device, the device form of the host reader's row gather, and the
// text feeder that runs both beside the step.
//
//   dfx_parse_criteo   ParseCriteo (difacto_amd/host/reader.cc; criteo_parser.h:40-92) over a
//                      chunk of whole lines already in device memory
//   dfx_gather_rows    GatherRows (reader.cc; the row copies of batch_reader.cc:29-78);
//                      dfx_gather_rows_valued: the same kernels with values and row flags
//   dfx_textfeed_*     pinned text slots, a loader stream, parsed chunks, a shuffle buffer and
//                      a ring of device batches (the producer half of sgd_learner.cc:289-314);
//                      its libsvm mode (dfx_parse_libsvm, libsvmparse.hip) is at the end
// The scans (block_scan, k_scan_*) are csrc/textscan.h, shared with libsvmparse.hip.
//
// The parser is parallel over bytes and cells, never one lane per row:
//   k_tp_tiles      every thread takes 16 bytes and marks its terminators ('\t', '\n'); a tile
//                   (4 KiB) reduces the tuple {newlines, start of the open cell, cells since the
//                   last newline}
//   k_scan_totals   one block scans the tile tuples (plain multi-launch scan: tile totals, a
//                   scan of the totals, apply — no look-back, nothing spins)
//   k_tp_cells      the same tuple scanned inside the tile gives every terminator its line, its
//                   cell number in the line and the cell's first byte; the thread owning the
//                   terminator hashes the cell (CityHash64, csrc/cityhash.h) into the line's
//                   slot table cells[line][0..40), parses a line's first cell as a label, and
//                   at a '\n' records the line's cell count
//   per line        which lines open a row (see below), the ids each line contributes; one
//                   scan of the pair gives every line its row and its place in index[]
//   k_tp_write      one wave per line compacts the line's non-empty cells into index[]
//
// Rows and lines.  ParseCriteo steps over the label's terminator whatever it is, so in a
// training file a line holding nothing but a label takes the NEXT line's cells as its feature
// columns 0, 1, ... and that line opens no row.  The device reproduces it: line l opens a row
// unless line l-1 opened one and had no tab, i.e. iff l - g(l) is even, g(l) the last line
// <= l that is 0 or follows a line with a tab (a max-scan over lines).  With is_train == 0
// every line is a row.
//
// The device result is either flagged (stat[2], needs_host) or equal to ParseCriteo's, never
// silently different.  The forms that raise the flag, and no others:
//   * a label cell that is not [+-]?[0-9]{1,9} filling the whole cell (an empty one too):
//     everything else atof accepts (fractions, exponents, hex, inf/nan, leading blanks) is
//     left to the host; the fast grammar is exact in double, so (float) of it is bit-identical
//   * a '\r' byte anywhere in the chunk
//   * an empty line
//   * a chunk whose last byte is not '\n'
// No byte outside [text, text + nbytes) is read; nothing past max_rows / max_nnz is written.
#include <algorithm>
#include <vector>

#include "cityhash.h"
#include "internal.h"
#include "textscan.h"

using namespace dfx;

namespace {

constexpr int kCols = 39;              // criteo feature columns (13 integer + 26 categorical)
constexpr int kLineSlots = 40;         // cells kept per line: a label and 39 columns

constexpr unsigned kFlagLabel = 1, kFlagCR = 2, kFlagEmptyLine = 4, kFlagTail = 8;

// {newlines, 1 + position of the last terminator (= first byte of the open cell; 0: none),
// terminators since the last newline}; combining is associative, left to right
struct TpT {
  uint32_t nl, last1, cafter;
};
struct TpOp {
  using T = TpT;
  __device__ static T id() { return TpT{0, 0, 0}; }
  __device__ static T f(const T& a, const T& b) {
    return TpT{a.nl + b.nl, b.last1 ? b.last1 : a.last1, b.nl ? b.cafter : a.cafter + b.cafter};
  }
};

// the parser's device counters (zeroed per call)
struct TpStat {
  unsigned int lines;  // '\n' bytes of the chunk
  unsigned int L;      // min(lines, linecap): the lines the per-line passes cover
  unsigned int L1;     // L + 1 (the scans' extra element carries the totals)
  unsigned int flags;  // kFlag* bits: needs_host
  TpT total;           // the byte pass's grand total
  uint2 rows_nnz;      // the line scan's grand total
};

// ---- the byte passes --------------------------------------------------------------------------
// masks of the terminators / newlines among the 16 bytes at pos (bytes at or past nbytes read
// as 0, no terminator); *cr: a '\r' among them
__device__ inline void tp_masks(const char* text, uint32_t nbytes, uint32_t pos, int aligned,
                                uint32_t* tmask, uint32_t* nmask, bool* cr) {
  uint32_t w[4] = {0, 0, 0, 0};
  if (aligned && (uint64_t)pos + kTpBytes <= nbytes) {
    const uint4 q = *reinterpret_cast<const uint4*>(text + pos);
    w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < kTpBytes; ++k)
      if ((uint64_t)pos + k < nbytes)
        w[k >> 2] |= (uint32_t)(uint8_t)text[pos + k] << (8 * (k & 3));
  }
  uint32_t t = 0, n = 0, r = 0;
#pragma unroll
  for (int k = 0; k < kTpBytes; ++k) {
    const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 255u;
    t |= (uint32_t)(c == '\t' || c == '\n') << k;
    n |= (uint32_t)(c == '\n') << k;
    r |= (uint32_t)(c == '\r');
  }
  *tmask = t;
  *nmask = n;
  *cr = r != 0;
}

__device__ inline TpT tp_tuple(uint32_t pos, uint32_t tmask, uint32_t nmask) {
  TpT v;
  v.nl = __popc(nmask);
  v.last1 = tmask ? pos + (31 - __clz(tmask)) + 1 : 0;
  v.cafter = nmask ? __popc(tmask >> (32 - __clz(nmask))) : __popc(tmask);
  return v;
}

__global__ __launch_bounds__(kNT) void k_tp_tiles(const char* text, uint32_t nbytes, int aligned,
                                                  TpT* tiles, TpStat* st) {
  __shared__ TpT lds[2 * kNT];
  const uint32_t pos = blockIdx.x * kTpTile + threadIdx.x * kTpBytes;
  uint32_t tmask, nmask;
  bool cr;
  tp_masks(text, nbytes, pos, aligned, &tmask, &nmask, &cr);
  if (cr) atomicOr(&st->flags, kFlagCR);
  TpT incl, excl, total;
  block_scan<TpOp, kNT>(tp_tuple(pos, tmask, nmask), lds, &incl, &excl, &total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ void k_tp_setlines(TpStat* st, const char* text, uint32_t nbytes, uint32_t linecap) {
  const uint32_t lines = st->total.nl;
  st->lines = lines;
  st->L = lines < linecap ? lines : linecap;
  st->L1 = st->L + 1;
  if (nbytes && text[nbytes - 1] != '\n') st->flags |= kFlagTail;
}

// the label's fast grammar: [+-]?[0-9]{1,9} filling the cell
__device__ inline bool tp_label(const char* s, uint32_t len, float* out) {
  if (len < 1 || len > 10) return false;
  uint32_t i = 0;
  bool neg = false;
  if (s[0] == '+' || s[0] == '-') {
    neg = s[0] == '-';
    i = 1;
  }
  const uint32_t nd = len - i;
  if (nd < 1 || nd > 9) return false;
  uint32_t a = 0;
  for (; i < len; ++i) {
    const uint32_t d = (uint32_t)(uint8_t)s[i] - (uint32_t)'0';
    if (d > 9) return false;
    a = a * 10 + d;
  }
  const float v = (float)a;  // round to nearest even, as (float)(double)a
  *out = neg ? -v : v;
  return true;
}

__global__ __launch_bounds__(kNT) void k_tp_cells(const char* text, uint32_t nbytes, int aligned,
                                                  const TpT* tiles, uint32_t linecap,
                                                  unsigned long long* cells, uint32_t* ncell,
                                                  float* lab, uint8_t* labok, TpStat* st) {
  __shared__ TpT lds[2 * kNT];
  const uint32_t pos = blockIdx.x * kTpTile + threadIdx.x * kTpBytes;
  uint32_t tmask, nmask;
  bool cr;
  tp_masks(text, nbytes, pos, aligned, &tmask, &nmask, &cr);
  TpT incl, excl, total;
  block_scan<TpOp, kNT>(tp_tuple(pos, tmask, nmask), lds, &incl, &excl, &total);
  const TpT in = TpOp::f(tiles[blockIdx.x], excl);
  uint32_t line = in.nl, start = in.last1, j = in.cafter;
  unsigned flags = 0;
  for (uint32_t m = tmask; m; m &= m - 1) {
    const int k = __ffs(m) - 1;
    const uint32_t p = pos + k, len = p - start;
    const bool isnl = (nmask >> k) & 1;
    if (line < linecap) {
      if (j < (uint32_t)kLineSlots)
        cells[(size_t)line * kLineSlots + j] =
            len ? (dfx_city::CityHash64(text + start, len) << 12) | 1ull : 0ull;
      if (j == 0) {
        float v = 0.f;
        labok[line] = tp_label(text + start, len, &v) ? 1 : 0;
        lab[line] = v;
      }
      if (isnl) {
        ncell[line] = j + 1;
        if (j == 0 && len == 0) flags |= kFlagEmptyLine;
      }
    }
    start = p + 1;
    if (isnl) {
      ++line;
      j = 0;
    } else {
      ++j;
    }
  }
  if (flags) atomicOr(&st->flags, flags);
}

// ---- the line passes --------------------------------------------------------------------------
// line l may open a row whatever came before it: it is line 0 or follows a line with a tab
struct MarkLoad {
  const uint32_t* ncell;
  __device__ uint32_t operator()(uint32_t i) const {
    return (i == 0 || ncell[i - 1] > 1) ? i : 0;
  }
};

// one wave per line: pair[l] = {opens a row, ids it contributes}; pair[L] = {0, 0}
__global__ __launch_bounds__(kNT) void k_tp_linecount(const unsigned long long* cells,
                                                      const uint32_t* ncell, const uint32_t* g,
                                                      const uint8_t* labok, int is_train,
                                                      uint2* pair, TpStat* st) {
  const uint32_t L = st->L;
  const uint64_t line64 = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (line64 > L) return;
  const uint32_t line = (uint32_t)line64;
  if (line == L) {
    if (lane == 0) pair[L] = make_uint2(0, 0);
    return;
  }
  const uint32_t opens = is_train ? (((line - g[line]) & 1u) == 0) : 1u;
  const uint32_t s = is_train ? opens : 0;  // the cells before column 0: the label
  const uint32_t j = lane + s;
  const bool valid = lane < (uint32_t)kCols && j < ncell[line] &&
                     (cells[(size_t)line * kLineSlots + j] & 1ull);
  const unsigned long long mask = __ballot(valid);
  if (lane == 0) {
    pair[line] = make_uint2(opens, (uint32_t)__popcll(mask));
    if (s && !labok[line]) atomicOr(&st->flags, kFlagLabel);
  }
}

// stat = {rows, nnz, needs_host, overflow}; with more lines than the caller's rows can hold
// (linecap) the per-line arrays do not cover the chunk: rows / nnz are then the upper bounds
// lines and 39 * lines, enough for a retry
__global__ void k_tp_finish(const TpStat* st, uint32_t linecap, int64_t max_rows, int64_t max_nnz,
                            int64_t* stat, uint64_t* offset) {
  int64_t rows = st->rows_nnz.x, nnz = st->rows_nnz.y;
  if (st->lines > linecap) {
    rows = st->lines;
    nnz = (int64_t)kCols * st->lines;
  }
  const int over = st->lines > linecap || rows > max_rows || nnz > max_nnz;
  stat[0] = rows;
  stat[1] = nnz;
  stat[2] = st->flags != 0;
  stat[3] = over;
  if (!over) offset[0] = 0;
}

// one wave per line: its non-empty cells of columns 0..38, compacted, to the row's place in
// index[]; the row's label and end offset
__global__ __launch_bounds__(kNT) void k_tp_write(const unsigned long long* cells,
                                                  const uint32_t* ncell, const float* lab,
                                                  const uint2* pair, int is_train,
                                                  const TpStat* st, const int64_t* stat,
                                                  uint64_t* offset, uint64_t* index,
                                                  float* label) {
  if (stat[3]) return;
  const uint32_t L = st->L;
  const uint64_t line64 = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (line64 >= L) return;
  const uint32_t line = (uint32_t)line64;
  const uint2 e0 = pair[line], e1 = pair[line + 1];
  const uint32_t opens = e1.x - e0.x;
  const uint32_t s = is_train ? opens : 0;
  const uint32_t row = opens ? e0.x : e0.x - 1;  // an absorbed line: the row before
  const uint32_t j = lane + s;
  unsigned long long v = 0;
  if (lane < (uint32_t)kCols && j < ncell[line]) v = cells[(size_t)line * kLineSlots + j];
  const bool valid = v & 1ull;
  const unsigned long long mask = __ballot(valid);
  if (valid) {
    const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    index[(size_t)e0.y + rank] = (v & ~0xfffull) | (unsigned long long)lane;
  }
  if (lane == 0) {
    if (opens) label[row] = is_train ? lab[line] : 0.f;
    const bool last = line + 1 == L || (pair[line + 2].x - e1.x) != 0;
    if (last) offset[(size_t)row + 1] = e1.y;
  }
}

// ---- the row gather -----------------------------------------------------------------------------
struct LenLoad {
  const uint64_t* off;
  const uint32_t* rows;
  uint64_t begin;
  uint32_t n;
  __device__ uint32_t operator()(uint32_t i) const {
    if (i >= n) return 0;  // the extra element: the total
    const uint64_t j = rows ? rows[i] : begin + i;
    return (uint32_t)(off[j + 1] - off[j]);
  }
};

// one wave per row: ids, label, the row's end offset rebased onto the destination's end;
// kValued: the values too (a source without values reads as ones, GatherRows's rule; no
// destination: dropped) and the row's flag byte
template <bool kValued>
__global__ __launch_bounds__(kNT) void k_tg_copy(const uint64_t* src_off, const uint64_t* src_idx,
                                                 const float* src_lab, const uint32_t* rows,
                                                 uint64_t begin, uint32_t n, const uint32_t* ex,
                                                 uint64_t* dst_off, uint64_t* dst_idx,
                                                 float* dst_lab, uint64_t r0,
                                                 const float* src_val, float* dst_val,
                                                 const uint8_t* src_flag, uint8_t* dst_flag) {
  const uint64_t i64 = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (i64 >= n) return;
  const uint32_t i = (uint32_t)i64;
  const uint64_t j = rows ? rows[i] : begin + i;
  const uint64_t base = r0 ? dst_off[r0] : 0;
  const uint64_t s0 = src_off[j], d0 = base + ex[i];
  const uint32_t len = ex[i + 1] - ex[i];
  for (uint32_t k = lane; k < len; k += 64) dst_idx[d0 + k] = src_idx[s0 + k];
  if (kValued && dst_val)
    for (uint32_t k = lane; k < len; k += 64) dst_val[d0 + k] = src_val ? src_val[s0 + k] : 1.f;
  if (lane == 0) {
    dst_off[r0 + i + 1] = base + ex[i + 1];
    dst_lab[r0 + i] = src_lab[j];
    if (kValued && dst_flag) dst_flag[r0 + i] = src_flag ? src_flag[j] : 0;
    if (r0 == 0 && i == 0) dst_off[0] = 0;
  }
}

template <bool kValued>
int gather_rows_on(Context* c, hipStream_t st, const uint64_t* src_offset,
                   const uint64_t* src_index, const float* src_label, const uint32_t* rows_dev,
                   int64_t begin, int64_t n, uint64_t* dst_offset, uint64_t* dst_index,
                   float* dst_label, int64_t r0, const float* src_value = nullptr,
                   float* dst_value = nullptr, const uint8_t* src_flag = nullptr,
                   uint8_t* dst_flag = nullptr) {
  DFX_CHECK_ARG(n >= 0 && n < (1ll << 31) && begin >= 0 && r0 >= 0, "gather_rows: bad range");
  if (n == 0) return DFX_OK;  // GatherRows: nothing appended, nothing touched
  DFX_CHECK_ARG(src_offset && src_index && src_label && dst_offset && dst_index && dst_label,
                "gather_rows: null array");
  const uint32_t n1 = (uint32_t)n + 1;
  DFX_TRY(c->tg_len.ensure((size_t)n1 * 4));
  DFX_TRY(c->tg_tot.ensure((size_t)blocks_for(n1, kNT) * 4));
  uint32_t* ex = c->tg_len.as<uint32_t>();
  uint32_t* tot = c->tg_tot.as<uint32_t>();
  const LenLoad load{src_offset, rows_dev, (uint64_t)begin, (uint32_t)n};
  hipLaunchKernelGGL((k_scan_reduce<AddOp, LenLoad>), dim3(blocks_for(n1, kNT)), dim3(kNT), 0, st,
                     load, (const uint32_t*)nullptr, n1, tot);
  hipLaunchKernelGGL((k_scan_totals<AddOp>), dim3(1), dim3(1024), 0, st, tot,
                     (const uint32_t*)nullptr, n1, (uint32_t)kNT, (uint32_t*)nullptr);
  hipLaunchKernelGGL((k_scan_apply<AddOp, LenLoad, false>), dim3(blocks_for(n1, kNT)), dim3(kNT),
                     0, st, load, (const uint32_t*)nullptr, n1, (const uint32_t*)tot, ex);
  hipLaunchKernelGGL(k_tg_copy<kValued>, dim3(blocks_for((uint64_t)n, kWavesPerBlock)), dim3(kNT),
                     0, st, src_offset, src_index, src_label, rows_dev, (uint64_t)begin,
                     (uint32_t)n, (const uint32_t*)ex, dst_offset, dst_index, dst_label,
                     (uint64_t)r0, src_value, dst_value, src_flag, dst_flag);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

// the parser's scratch: the context's own set (dfx_parse_criteo, on the input stream) or a text
// feeder's (its parses run on a stream of their own)
struct TpScratch {
  DevBuf *tiles, *cells, *lines, *pair, *tot, *stat;
};

int parse_criteo_on(const TpScratch& ws, hipStream_t st, const char* text, int64_t nbytes,
                    int is_train, int64_t max_rows, int64_t max_nnz, uint64_t* offset,
                    uint64_t* index, float* label, int64_t* stat_dev) {
  DFX_CHECK_ARG(nbytes >= 0 && nbytes < (1ll << 31),
                "parse_criteo: positions are 32-bit, nbytes must be in [0, 2^31)");
  DFX_CHECK_ARG(max_rows >= 0 && max_nnz >= 0 && offset && stat_dev && (text || nbytes == 0) &&
                    (label || max_rows == 0) && (index || max_nnz == 0),
                "parse_criteo: bad argument");
  is_train = is_train ? 1 : 0;
  // the lines the per-line arrays cover: a row is one line, or two when a training line holds
  // only its label; never more lines than bytes
  const int64_t rows_cl = std::min<int64_t>(max_rows, 1ll << 31);
  const uint32_t linecap =
      (uint32_t)std::min<int64_t>(is_train ? 2 * rows_cl + 1 : rows_cl, nbytes);
  const uint32_t ntiles = blocks_for((uint64_t)nbytes, kTpTile);
  const uint32_t nl1 = linecap + 1;
  DFX_TRY(ws.tiles->ensure((size_t)ntiles * sizeof(TpT)));
  DFX_TRY(ws.cells->ensure((size_t)linecap * kLineSlots * 8));
  // per line: ncell (u32), lab (f32), g (u32), labok (u8)
  DFX_TRY(ws.lines->ensure((size_t)nl1 * 13));
  DFX_TRY(ws.pair->ensure((size_t)nl1 * sizeof(uint2)));
  DFX_TRY(ws.tot->ensure((size_t)blocks_for(nl1, kNT) * sizeof(uint2)));
  DFX_TRY(ws.stat->ensure(sizeof(TpStat)));
  TpT* tiles = ws.tiles->as<TpT>();
  unsigned long long* cells = ws.cells->as<unsigned long long>();
  uint32_t* ncell = ws.lines->as<uint32_t>();
  float* lab = reinterpret_cast<float*>(ncell + nl1);
  uint32_t* g = ncell + 2 * (size_t)nl1;
  uint8_t* labok = reinterpret_cast<uint8_t*>(ncell + 3 * (size_t)nl1);
  uint2* pair = ws.pair->as<uint2>();
  TpStat* ds = ws.stat->as<TpStat>();
  const int aligned = (reinterpret_cast<uintptr_t>(text) & 15) == 0;
  DFX_HIP(hipMemsetAsync(ds, 0, sizeof(TpStat), st));
  if (nbytes > 0) {
    hipLaunchKernelGGL(k_tp_tiles, dim3(ntiles), dim3(kNT), 0, st, text, (uint32_t)nbytes, aligned,
                       tiles, ds);
    hipLaunchKernelGGL((k_scan_totals<TpOp>), dim3(1), dim3(1024), 0, st, tiles,
                       (const uint32_t*)nullptr, (uint32_t)nbytes, (uint32_t)kTpTile, &ds->total);
  }
  hipLaunchKernelGGL(k_tp_setlines, dim3(1), dim3(1), 0, st, ds, text, (uint32_t)nbytes, linecap);
  if (nbytes > 0 && linecap > 0) {
    hipLaunchKernelGGL(k_tp_cells, dim3(ntiles), dim3(kNT), 0, st, text, (uint32_t)nbytes, aligned,
                       (const TpT*)tiles, linecap, cells, ncell, lab, labok, ds);
    if (is_train) {  // g: the last line at or before l that opens a row whatever came before
      uint32_t* tot = ws.tot->as<uint32_t>();
      const MarkLoad load{ncell};
      hipLaunchKernelGGL((k_scan_reduce<MaxOp, MarkLoad>), dim3(blocks_for(linecap, kNT)),
                         dim3(kNT), 0, st, load, (const uint32_t*)&ds->L, linecap, tot);
      hipLaunchKernelGGL((k_scan_totals<MaxOp>), dim3(1), dim3(1024), 0, st, tot,
                         (const uint32_t*)&ds->L, linecap, (uint32_t)kNT, (uint32_t*)nullptr);
      hipLaunchKernelGGL((k_scan_apply<MaxOp, MarkLoad, true>), dim3(blocks_for(linecap, kNT)),
                         dim3(kNT), 0, st, load, (const uint32_t*)&ds->L, linecap,
                         (const uint32_t*)tot, g);
    }
  }
  {
    uint2* tot = ws.tot->as<uint2>();
    const PtrLoad<uint2> load{pair};
    hipLaunchKernelGGL(k_tp_linecount, dim3(blocks_for(nl1, kWavesPerBlock)), dim3(kNT), 0, st,
                       (const unsigned long long*)cells, (const uint32_t*)ncell,
                       (const uint32_t*)g, (const uint8_t*)labok, is_train, pair, ds);
    hipLaunchKernelGGL((k_scan_reduce<Add2Op, PtrLoad<uint2>>), dim3(blocks_for(nl1, kNT)),
                       dim3(kNT), 0, st, load, (const uint32_t*)&ds->L1, nl1, tot);
    hipLaunchKernelGGL((k_scan_totals<Add2Op>), dim3(1), dim3(1024), 0, st, tot,
                       (const uint32_t*)&ds->L1, nl1, (uint32_t)kNT, &ds->rows_nnz);
    hipLaunchKernelGGL((k_scan_apply<Add2Op, PtrLoad<uint2>, false>), dim3(blocks_for(nl1, kNT)),
                       dim3(kNT), 0, st, load, (const uint32_t*)&ds->L1, nl1, (const uint2*)tot,
                       pair);
  }
  hipLaunchKernelGGL(k_tp_finish, dim3(1), dim3(1), 0, st, (const TpStat*)ds, linecap, max_rows,
                     max_nnz, stat_dev, offset);
  if (linecap > 0)
    hipLaunchKernelGGL(k_tp_write, dim3(blocks_for(linecap, kWavesPerBlock)), dim3(kNT), 0, st,
                       (const unsigned long long*)cells, (const uint32_t*)ncell, (const float*)lab,
                       (const uint2*)pair, is_train, (const TpStat*)ds, (const int64_t*)stat_dev,
                       offset, index, label);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

int capacity_status(const int64_t* stat) {
  if (!stat[3]) return DFX_OK;
  set_error("parse_criteo: the chunk needs " + std::to_string(stat[0]) + " rows and " +
            std::to_string(stat[1]) + " ids, more than the caller's capacity");
  return DFX_ERR_CAPACITY;
}

}  // namespace

extern "C" int dfx_parse_criteo(dfx_ctx* ctx, const char* text_dev, int64_t nbytes, int is_train,
                                int64_t max_rows, int64_t max_nnz, uint64_t* offset,
                                uint64_t* index, float* label, int64_t* stat_dev) {
  DFX_CHECK_ARG(ctx, "null ctx");
  DFX_HIP(hipSetDevice(ctx->c.device));
  Context* c = &ctx->c;
  const TpScratch ws{&c->tp_tiles, &c->tp_cells, &c->tp_lines, &c->tp_pair, &c->tp_tot,
                     &c->tp_stat};
  return parse_criteo_on(ws, input_stream(c), text_dev, nbytes, is_train, max_rows, max_nnz,
                         offset, index, label, stat_dev);
}

extern "C" int dfx_parse_criteo_wait(dfx_ctx* ctx, const int64_t* stat_dev, int64_t* stat) {
  DFX_CHECK_ARG(ctx && stat_dev && stat, "parse_criteo_wait: null argument");
  hipStream_t st = input_stream(&ctx->c);
  DFX_HIP(hipMemcpyAsync(stat, stat_dev, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  DFX_HIP(hipStreamSynchronize(st));
  return capacity_status(stat);
}

extern "C" int dfx_gather_rows(dfx_ctx* ctx, const uint64_t* src_offset, const uint64_t* src_index,
                               const float* src_label, const uint32_t* rows_dev, int64_t begin,
                               int64_t n, uint64_t* dst_offset, uint64_t* dst_index,
                               float* dst_label, int64_t r0) {
  DFX_CHECK_ARG(ctx, "null ctx");
  DFX_HIP(hipSetDevice(ctx->c.device));
  return gather_rows_on<false>(&ctx->c, input_stream(&ctx->c), src_offset, src_index, src_label,
                               rows_dev, begin, n, dst_offset, dst_index, dst_label, r0);
}

extern "C" int dfx_gather_rows_valued(dfx_ctx* ctx, const uint64_t* src_offset,
                                      const uint64_t* src_index, const float* src_value,
                                      const float* src_label, const uint8_t* src_rowflag,
                                      const uint32_t* rows_dev, int64_t begin, int64_t n,
                                      uint64_t* dst_offset, uint64_t* dst_index, float* dst_value,
                                      float* dst_label, uint8_t* dst_rowflag, int64_t r0) {
  DFX_CHECK_ARG(ctx, "null ctx");
  DFX_HIP(hipSetDevice(ctx->c.device));
  return gather_rows_on<true>(&ctx->c, input_stream(&ctx->c), src_offset, src_index, src_label,
                              rows_dev, begin, n, dst_offset, dst_index, dst_label, r0, src_value,
                              dst_value, src_rowflag, dst_rowflag);
}

// ---- the text feeder ----------------------------------------------------------------------------
// A CSR of criteo rows on the device: at most 39 ids per row, so rows alone size it.  In the
// libsvm mode (ensure_valued) it also holds values and row flags and has an nnz capacity of its
// own, which grows on demand.
namespace {
struct DevCsr {
  uint64_t *off = nullptr, *idx = nullptr;
  float* lab = nullptr;
  int64_t cap = 0;  // rows
  float* val = nullptr;  // the libsvm mode
  uint8_t* flag = nullptr;
  int64_t nnz_cap = 0;
  // room for rows / nnz; growth is x1.25 and keeps the first keep_rows rows and keep_nnz
  // features: copied on st, in order behind whatever st holds that reads or writes the old
  // arrays, and joined before they are freed
  int ensure_valued(int64_t rows, int64_t nnz, hipStream_t st = nullptr, int64_t keep_rows = 0,
                    int64_t keep_nnz = 0) {
    if (off && val && rows <= cap && nnz <= nnz_cap) return DFX_OK;
    const int64_t nr = off && rows <= cap ? cap : std::max<int64_t>(rows + rows / 4, 16);
    const int64_t nn = val && nnz <= nnz_cap ? nnz_cap : std::max<int64_t>(nnz + nnz / 4, 64);
    DevCsr n;
    DFX_HIP(hipMalloc(&n.off, (size_t)(nr + 1) * 8));
    DFX_HIP(hipMalloc(&n.idx, (size_t)nn * 8));
    DFX_HIP(hipMalloc(&n.lab, (size_t)nr * 4));
    DFX_HIP(hipMalloc(&n.val, (size_t)nn * 4));
    DFX_HIP(hipMalloc(&n.flag, (size_t)nr));
    n.cap = nr;
    n.nnz_cap = nn;
    if (st && off && val && (keep_rows || keep_nnz)) {
      const hipMemcpyKind k = hipMemcpyDeviceToDevice;
      DFX_HIP(hipMemcpyAsync(n.off, off, (size_t)(keep_rows + 1) * 8, k, st));
      if (keep_rows) DFX_HIP(hipMemcpyAsync(n.lab, lab, (size_t)keep_rows * 4, k, st));
      if (keep_rows) DFX_HIP(hipMemcpyAsync(n.flag, flag, (size_t)keep_rows, k, st));
      if (keep_nnz) DFX_HIP(hipMemcpyAsync(n.idx, idx, (size_t)keep_nnz * 8, k, st));
      if (keep_nnz) DFX_HIP(hipMemcpyAsync(n.val, val, (size_t)keep_nnz * 4, k, st));
    }
    if (st) DFX_HIP(hipStreamSynchronize(st));
    release();
    *this = n;
    return DFX_OK;
  }
  int ensure(int64_t rows) {
    if (rows <= cap && off) return DFX_OK;
    release();
    rows = std::max<int64_t>(rows + rows / 4, 16);
    DFX_HIP(hipMalloc(&off, (size_t)(rows + 1) * 8));
    DFX_HIP(hipMalloc(&idx, (size_t)rows * kCols * 8));
    DFX_HIP(hipMalloc(&lab, (size_t)rows * 4));
    cap = rows;
    return DFX_OK;
  }
  void release() {
    for (void* p : {(void*)off, (void*)idx, (void*)lab, (void*)val, (void*)flag})
      if (p) (void)hipFree(p);
    off = idx = nullptr;
    lab = val = nullptr;
    flag = nullptr;
    cap = nnz_cap = 0;
  }
};
}  // namespace

// Two streams: the gathers run on `stream`, the context's input stream, which a step waits
// for; uploads, parses and the copies back run on `up_stream`, so a later chunk's upload does
// not sit between a batch's gathers and its step.  Events order the two: a gather waits for
// its source chunk's `parsed`, a parse into a slot for the slot's last gather (`gathered`).
struct dfx_textfeed {
  dfx_ctx* ctx = nullptr;
  hipStream_t stream = nullptr, up_stream = nullptr;
  DevBuf tp[6];  // the parser's scratch on up_stream
  struct Slot {
    char *h_text = nullptr, *d_text = nullptr;
    int64_t text_cap = 0;
    DevCsr csr;
    uint64_t* h_off = nullptr;  // pinned mirrors of the parsed offsets / labels / counts
    float* h_lab = nullptr;
    uint8_t* h_flag = nullptr;  // the libsvm mode: the row flags
    int64_t mirror_cap = 0;
    int64_t *d_stat = nullptr, *h_stat = nullptr;
    int64_t rows = 0, nnz = 0;
    hipEvent_t parsed = nullptr, consumed = nullptr, gathered = nullptr;
  };
  struct Ring {
    DevCsr csr;
    uint32_t *h_rows = nullptr, *d_rows = nullptr;  // the batch's row lists, appended
    int64_t used = 0;
    int64_t nnz = 0;  // the libsvm mode: features gathered into the batch so far
    hipEvent_t consumed = nullptr;
  };
  std::vector<Slot> slot;
  std::vector<Ring> ring;
  DevCsr shuf;
  int64_t shuf_nnz = 0;  // the libsvm mode: features in the shuffle buffer
  int64_t batch_rows = 0;
  int cur = -1;
  int format = DFX_TEXT_CRITEO;
};

extern "C" int dfx_textfeed_destroy(dfx_textfeed* f) {
  if (!f) return DFX_OK;
  if (f->stream) (void)hipStreamSynchronize(f->stream);
  if (f->up_stream) (void)hipStreamSynchronize(f->up_stream);
  (void)hipDeviceSynchronize();
  for (DevBuf& b : f->tp) b.release();
  for (auto& s : f->slot) {
    for (void* p : {(void*)s.h_text, (void*)s.h_off, (void*)s.h_lab, (void*)s.h_stat,
                    (void*)s.h_flag})
      if (p) (void)hipHostFree(p);
    for (void* p : {(void*)s.d_text, (void*)s.d_stat})
      if (p) (void)hipFree(p);
    s.csr.release();
    for (hipEvent_t e : {s.parsed, s.consumed, s.gathered})
      if (e) (void)hipEventDestroy(e);
  }
  for (auto& r : f->ring) {
    r.csr.release();
    if (r.h_rows) (void)hipHostFree(r.h_rows);
    if (r.d_rows) (void)hipFree(r.d_rows);
    if (r.consumed) (void)hipEventDestroy(r.consumed);
  }
  f->shuf.release();
  if (f->ctx) (void)dfx_ctx_set_input_stream(f->ctx, nullptr);
  if (f->stream) (void)hipStreamDestroy(f->stream);
  if (f->up_stream) (void)hipStreamDestroy(f->up_stream);
  delete f;
  return DFX_OK;
}

extern "C" int dfx_textfeed_create_fmt(dfx_ctx* ctx, int nslots, int nring, int64_t batch_rows,
                                       int64_t shuf_rows, int format, dfx_textfeed** out) {
  DFX_CHECK_ARG(ctx && out && nslots >= 2 && nslots <= 8 && nring >= 2 && nring <= 8 &&
                    batch_rows > 0 && batch_rows < (1ll << 31) && shuf_rows >= 0 &&
                    (format == DFX_TEXT_CRITEO || format == DFX_TEXT_LIBSVM),
                "textfeed_create: bad argument");
  DFX_HIP(hipSetDevice(ctx->c.device));
  dfx_textfeed* f = new dfx_textfeed();
  f->ctx = ctx;
  f->format = format;
  const bool valued = format == DFX_TEXT_LIBSVM;
  f->batch_rows = batch_rows;
  f->slot.resize((size_t)nslots);
  f->ring.resize((size_t)nring);
  auto fail = [&](const char* what) {
    set_error(std::string("textfeed_create: ") + what);
    dfx_textfeed_destroy(f);
    return DFX_ERR_HIP;
  };
  if (hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&f->up_stream, hipStreamNonBlocking) != hipSuccess)
    return fail("stream");
  for (auto& s : f->slot) {
    if (hipEventCreateWithFlags(&s.parsed, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s.gathered, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s.consumed, hipEventDisableTiming) != hipSuccess)
      return fail("event");
    if (hipMalloc(&s.d_stat, 4 * sizeof(int64_t)) != hipSuccess ||
        hipHostMalloc(&s.h_stat, 4 * sizeof(int64_t), hipHostMallocDefault) != hipSuccess)
      return fail("counters");
  }
  for (auto& r : f->ring) {
    if (hipEventCreateWithFlags(&r.consumed, hipEventDisableTiming) != hipSuccess)
      return fail("event");
    if ((valued ? r.csr.ensure_valued(batch_rows, batch_rows * kCols)
                : r.csr.ensure(batch_rows)) != DFX_OK)
      return fail("device batch");
    if (hipHostMalloc(&r.h_rows, (size_t)batch_rows * 4, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&r.d_rows, (size_t)batch_rows * 4) != hipSuccess)
      return fail("row lists");
  }
  if (shuf_rows > 0 && (valued ? f->shuf.ensure_valued(shuf_rows, shuf_rows * kCols)
                               : f->shuf.ensure(shuf_rows)) != DFX_OK)
    return fail("shuffle buffer");
  int rc = dfx_ctx_set_input_stream(ctx, f->stream);
  if (rc != DFX_OK) {
    dfx_textfeed_destroy(f);
    return rc;
  }
  *out = f;
  return DFX_OK;
}

extern "C" int dfx_textfeed_create(dfx_ctx* ctx, int nslots, int nring, int64_t batch_rows,
                                   int64_t shuf_rows, dfx_textfeed** out) {
  return dfx_textfeed_create_fmt(ctx, nslots, nring, batch_rows, shuf_rows, DFX_TEXT_CRITEO, out);
}

#define DFX_FEED_SLOT(f, s, what) \
  DFX_CHECK_ARG((f) && (s) >= 0 && (s) < (int)(f)->slot.size(), what ": bad slot")
#define DFX_FEED_FMT(f, fmt, what) \
  DFX_CHECK_ARG((f) && (f)->format == (fmt), what ": not this feed's format")

extern "C" int dfx_textfeed_text(dfx_textfeed* f, int slot, int64_t bytes, char** pinned) {
  DFX_FEED_SLOT(f, slot, "textfeed_text");
  DFX_CHECK_ARG(pinned && bytes >= 0 && bytes < (1ll << 31), "textfeed_text: bad argument");
  DFX_HIP(hipSetDevice(f->ctx->c.device));
  auto& s = f->slot[slot];
  if (bytes > s.text_cap || !s.h_text) {
    if (s.h_text) DFX_HIP(hipHostFree(s.h_text));
    if (s.d_text) DFX_HIP(hipFree(s.d_text));
    s.h_text = s.d_text = nullptr;
    s.text_cap = 0;
    const int64_t cap = std::max<int64_t>(bytes + bytes / 8, 4096);
    DFX_HIP(hipHostMalloc(&s.h_text, (size_t)cap, hipHostMallocDefault));
    DFX_HIP(hipMalloc(&s.d_text, (size_t)cap));
    s.text_cap = cap;
  }
  *pinned = s.h_text;
  return DFX_OK;
}

static int feed_slot_rows(dfx_textfeed* f, dfx_textfeed::Slot& s, int64_t rows) {
  DFX_TRY(s.csr.ensure(rows));
  if (rows > s.mirror_cap || !s.h_off) {
    if (s.h_off) DFX_HIP(hipHostFree(s.h_off));
    if (s.h_lab) DFX_HIP(hipHostFree(s.h_lab));
    s.h_off = nullptr;
    s.h_lab = nullptr;
    s.mirror_cap = 0;
    DFX_HIP(hipHostMalloc(&s.h_off, (size_t)(s.csr.cap + 1) * 8, hipHostMallocDefault));
    DFX_HIP(hipHostMalloc(&s.h_lab, (size_t)s.csr.cap * 4, hipHostMallocDefault));
    s.mirror_cap = s.csr.cap;
  }
  (void)f;
  return DFX_OK;
}

extern "C" int dfx_textfeed_submit(dfx_textfeed* f, int slot, int64_t nbytes, int is_train,
                                   int64_t max_rows) {
  DFX_FEED_SLOT(f, slot, "textfeed_submit");
  DFX_FEED_FMT(f, DFX_TEXT_CRITEO, "textfeed_submit");
  auto& s = f->slot[slot];
  DFX_CHECK_ARG(nbytes >= 0 && nbytes <= s.text_cap && max_rows >= 0,
                "textfeed_submit: more bytes than dfx_textfeed_text reserved");
  DFX_HIP(hipSetDevice(f->ctx->c.device));
  DFX_TRY(feed_slot_rows(f, s, max_rows));
  hipStream_t up = f->up_stream;
  // the gathers that read the slot's previous chunk, and a step that took it as its batch,
  // must be past the device
  DFX_HIP(hipStreamWaitEvent(up, s.gathered, 0));
  DFX_HIP(hipStreamWaitEvent(up, s.consumed, 0));
  if (nbytes)
    DFX_HIP(hipMemcpyAsync(s.d_text, s.h_text, (size_t)nbytes, hipMemcpyHostToDevice, up));
  const TpScratch ws{&f->tp[0], &f->tp[1], &f->tp[2], &f->tp[3], &f->tp[4], &f->tp[5]};
  DFX_TRY(parse_criteo_on(ws, up, s.d_text, nbytes, is_train, max_rows, max_rows * kCols,
                          s.csr.off, s.csr.idx, s.csr.lab, s.d_stat));
  // offsets and labels (12 bytes a row) for the batch planner, the counts
  DFX_HIP(hipMemcpyAsync(s.h_off, s.csr.off, (size_t)(max_rows + 1) * 8, hipMemcpyDeviceToHost,
                         up));
  if (max_rows)
    DFX_HIP(hipMemcpyAsync(s.h_lab, s.csr.lab, (size_t)max_rows * 4, hipMemcpyDeviceToHost, up));
  DFX_HIP(hipMemcpyAsync(s.h_stat, s.d_stat, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, up));
  DFX_HIP(hipEventRecord(s.parsed, up));
  return DFX_OK;
}

extern "C" int dfx_textfeed_wait(dfx_textfeed* f, int slot, int64_t* stat,
                                 const uint64_t** offset_host, const float** label_host) {
  DFX_FEED_SLOT(f, slot, "textfeed_wait");
  DFX_CHECK_ARG(stat, "textfeed_wait: null argument");
  auto& s = f->slot[slot];
  DFX_HIP(hipEventSynchronize(s.parsed));
  for (int i = 0; i < 4; ++i) stat[i] = s.h_stat[i];
  s.rows = stat[0];
  s.nnz = stat[1];
  if (offset_host) *offset_host = s.h_off;
  if (label_host) *label_host = s.h_lab;
  return capacity_status(stat);
}

extern "C" int dfx_textfeed_upload(dfx_textfeed* f, int slot, int64_t rows, int64_t nnz,
                                   const uint64_t* offset, const uint64_t* index,
                                   const float* label) {
  DFX_FEED_SLOT(f, slot, "textfeed_upload");
  DFX_FEED_FMT(f, DFX_TEXT_CRITEO, "textfeed_upload");
  DFX_CHECK_ARG(rows >= 0 && nnz >= 0 && nnz <= rows * kCols && offset && (index || !nnz) &&
                    (label || !rows),
                "textfeed_upload: bad argument");
  auto& s = f->slot[slot];
  DFX_HIP(hipSetDevice(f->ctx->c.device));
  hipStream_t up = f->up_stream;
  if (rows > s.csr.cap) {
    DFX_HIP(hipStreamSynchronize(up));
    DFX_TRY(feed_slot_rows(f, s, rows));
  }
  // after the slot's own parse (dfx_textfeed_wait joined it); the gathers wait for `parsed`
  DFX_HIP(hipMemcpyAsync(s.csr.off, offset, (size_t)(rows + 1) * 8, hipMemcpyHostToDevice, up));
  if (nnz) DFX_HIP(hipMemcpyAsync(s.csr.idx, index, (size_t)nnz * 8, hipMemcpyHostToDevice, up));
  if (rows) {
    DFX_HIP(hipMemcpyAsync(s.csr.lab, label, (size_t)rows * 4, hipMemcpyHostToDevice, up));
    std::copy(label, label + rows, s.h_lab);
  }
  std::copy(offset, offset + rows + 1, s.h_off);
  // the caller's arrays are pageable: staged before the calls return
  DFX_HIP(hipEventRecord(s.parsed, up));
  s.rows = rows;
  s.nnz = nnz;
  return DFX_OK;
}

extern "C" int dfx_textfeed_batch_begin(dfx_textfeed* f) {
  DFX_CHECK_ARG(f, "textfeed_batch_begin: null argument");
  f->cur = (f->cur + 1) % (int)f->ring.size();
  auto& r = f->ring[f->cur];
  // the step that consumed this ring entry a round ago must be past the device (its row lists
  // are pinned host memory the gathers' copies read)
  DFX_HIP(hipEventSynchronize(r.consumed));
  r.used = 0;
  return DFX_OK;
}

extern "C" int dfx_textfeed_gather(dfx_textfeed* f, int src, int to_batch, const uint32_t* rows,
                                   int64_t begin, int64_t n, int64_t r0) {
  DFX_CHECK_ARG(f && src >= -1 && src < (int)f->slot.size() && n >= 0 && r0 >= 0 && begin >= 0,
                "textfeed_gather: bad argument");
  DFX_CHECK_ARG(!to_batch || f->cur >= 0, "textfeed_gather: no batch begun");
  DFX_CHECK_ARG(src >= 0 || to_batch, "textfeed_gather: the shuffle buffer onto itself");
  DFX_FEED_FMT(f, DFX_TEXT_CRITEO, "textfeed_gather");
  if (n == 0) return DFX_OK;
  DFX_HIP(hipSetDevice(f->ctx->c.device));
  const DevCsr& S = src >= 0 ? f->slot[src].csr : f->shuf;
  const DevCsr& D = to_batch ? f->ring[f->cur].csr : f->shuf;
  DFX_CHECK_ARG(r0 + n <= D.cap, "textfeed_gather: more rows than the destination holds");
  const uint32_t* rows_dev = nullptr;
  if (rows) {
    DFX_CHECK_ARG(to_batch, "textfeed_gather: row lists go to the batch");
    auto& r = f->ring[f->cur];
    DFX_CHECK_ARG(r.used + n <= f->batch_rows, "textfeed_gather: row lists past the batch size");
    std::copy(rows, rows + n, r.h_rows + r.used);
    DFX_HIP(hipMemcpyAsync(r.d_rows + r.used, r.h_rows + r.used, (size_t)n * 4,
                           hipMemcpyHostToDevice, f->stream));
    rows_dev = r.d_rows + r.used;
    r.used += n;
  }
  if (src >= 0) DFX_HIP(hipStreamWaitEvent(f->stream, f->slot[src].parsed, 0));
  DFX_TRY(gather_rows_on<false>(&f->ctx->c, f->stream, S.off, S.idx, S.lab, rows_dev, begin, n,
                                D.off, D.idx, D.lab, r0));
  if (src >= 0) DFX_HIP(hipEventRecord(f->slot[src].gathered, f->stream));
  return DFX_OK;
}

extern "C" int dfx_textfeed_batch_end(dfx_textfeed* f, int64_t rows, int64_t nnz, dfx_batch* out) {
  DFX_CHECK_ARG(f && out && f->cur >= 0 && rows >= 0 && nnz >= 0, "textfeed_batch_end: bad argument");
  const DevCsr& D = f->ring[f->cur].csr;
  *out = dfx_batch{};
  out->size = rows;
  out->nnz = nnz;
  out->offset = D.off;
  out->index = D.idx;
  out->label = D.lab;
  return DFX_OK;
}

extern "C" int dfx_textfeed_consumed(dfx_textfeed* f) {
  DFX_CHECK_ARG(f && f->cur >= 0, "textfeed_consumed: no batch begun");
  DFX_HIP(hipEventRecord(f->ring[f->cur].consumed, f->ctx->c.stream));
  return DFX_OK;
}

extern "C" int dfx_textfeed_slot_batch(dfx_textfeed* f, int slot, dfx_batch* out) {
  DFX_FEED_SLOT(f, slot, "textfeed_slot_batch");
  DFX_CHECK_ARG(out, "textfeed_slot_batch: null argument");
  const auto& s = f->slot[slot];
  // the step waits for the input stream, the input stream for the chunk's parse
  DFX_HIP(hipStreamWaitEvent(f->stream, s.parsed, 0));
  *out = dfx_batch{};
  out->size = s.rows;
  out->nnz = s.nnz;
  out->offset = s.csr.off;
  out->index = s.csr.idx;
  out->label = s.csr.lab;
  return DFX_OK;
}

extern "C" int dfx_textfeed_slot_consumed(dfx_textfeed* f, int slot) {
  DFX_FEED_SLOT(f, slot, "textfeed_slot_consumed");
  DFX_HIP(hipEventRecord(f->slot[slot].consumed, f->ctx->c.stream));
  return DFX_OK;
}

// ---- the libsvm mode ------------------------------------------------------------------------------
// The same slots, shuffle buffer and ring with values and row flags beside the ids.  A row has
// any number of features, so every CSR has an nnz capacity of its own: a slot's is the caller's
// bound for its chunk, the shuffle buffer's and a ring entry's grow on demand (x1.25) and keep
// their contents.
static int feed_slot_valued(dfx_textfeed::Slot& s, int64_t rows, int64_t nnz) {
  DFX_TRY(s.csr.ensure_valued(rows, nnz));
  if (s.csr.cap > s.mirror_cap || !s.h_off || !s.h_flag) {
    for (void* p : {(void*)s.h_off, (void*)s.h_lab, (void*)s.h_flag})
      if (p) DFX_HIP(hipHostFree(p));
    s.h_off = nullptr;
    s.h_lab = nullptr;
    s.h_flag = nullptr;
    s.mirror_cap = 0;
    DFX_HIP(hipHostMalloc(&s.h_off, (size_t)(s.csr.cap + 1) * 8, hipHostMallocDefault));
    DFX_HIP(hipHostMalloc(&s.h_lab, (size_t)s.csr.cap * 4, hipHostMallocDefault));
    DFX_HIP(hipHostMalloc(&s.h_flag, (size_t)s.csr.cap, hipHostMallocDefault));
    s.mirror_cap = s.csr.cap;
  }
  return DFX_OK;
}

extern "C" int dfx_textfeed_submit_libsvm(dfx_textfeed* f, int slot, int64_t nbytes,
                                          int64_t max_rows, int64_t max_nnz) {
  DFX_FEED_SLOT(f, slot, "textfeed_submit_libsvm");
  DFX_FEED_FMT(f, DFX_TEXT_LIBSVM, "textfeed_submit_libsvm");
  auto& s = f->slot[slot];
  DFX_CHECK_ARG(nbytes >= 0 && nbytes <= s.text_cap && max_rows >= 0 && max_nnz >= 0,
                "textfeed_submit_libsvm: more bytes than dfx_textfeed_text reserved");
  DFX_HIP(hipSetDevice(f->ctx->c.device));
  DFX_TRY(feed_slot_valued(s, max_rows, max_nnz));
  hipStream_t up = f->up_stream;
  DFX_HIP(hipStreamWaitEvent(up, s.gathered, 0));
  DFX_HIP(hipStreamWaitEvent(up, s.consumed, 0));
  if (nbytes)
    DFX_HIP(hipMemcpyAsync(s.d_text, s.h_text, (size_t)nbytes, hipMemcpyHostToDevice, up));
  DFX_TRY(parse_libsvm_on(&f->tp[0], &f->tp[5], up, s.d_text, nbytes, max_rows, max_nnz,
                          s.csr.off, s.csr.idx, s.csr.val, s.csr.lab, s.csr.flag, s.d_stat));
  // offsets, labels and row flags (13 bytes a row) for the batch planner, the counts
  DFX_HIP(hipMemcpyAsync(s.h_off, s.csr.off, (size_t)(max_rows + 1) * 8, hipMemcpyDeviceToHost,
                         up));
  if (max_rows) {
    DFX_HIP(hipMemcpyAsync(s.h_lab, s.csr.lab, (size_t)max_rows * 4, hipMemcpyDeviceToHost, up));
    DFX_HIP(hipMemcpyAsync(s.h_flag, s.csr.flag, (size_t)max_rows, hipMemcpyDeviceToHost, up));
  }
  DFX_HIP(hipMemcpyAsync(s.h_stat, s.d_stat, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, up));
  DFX_HIP(hipEventRecord(s.parsed, up));
  return DFX_OK;
}

extern "C" int dfx_textfeed_wait_valued(dfx_textfeed* f, int slot, int64_t* stat,
                                        const uint64_t** offset_host, const float** label_host,
                                        const uint8_t** rowflag_host) {
  DFX_FEED_SLOT(f, slot, "textfeed_wait_valued");
  if (rowflag_host) *rowflag_host = f->slot[slot].h_flag;
  return dfx_textfeed_wait(f, slot, stat, offset_host, label_host);
}

extern "C" int dfx_textfeed_upload_valued(dfx_textfeed* f, int slot, int64_t rows, int64_t nnz,
                                          const uint64_t* offset, const uint64_t* index,
                                          const float* value, const float* label) {
  DFX_FEED_SLOT(f, slot, "textfeed_upload_valued");
  DFX_FEED_FMT(f, DFX_TEXT_LIBSVM, "textfeed_upload_valued");
  DFX_CHECK_ARG(rows >= 0 && nnz >= 0 && offset && ((index && value) || !nnz) &&
                    (label || !rows) && offset[0] == 0 && (int64_t)offset[rows] == nnz,
                "textfeed_upload_valued: bad argument");
  auto& s = f->slot[slot];
  DFX_HIP(hipSetDevice(f->ctx->c.device));
  hipStream_t up = f->up_stream;
  if (rows > s.csr.cap || nnz > s.csr.nnz_cap || !s.h_flag) {
    DFX_HIP(hipStreamSynchronize(up));
    DFX_TRY(feed_slot_valued(s, rows, nnz));
  }
  // after the slot's own parse (dfx_textfeed_wait joined it); the gathers wait for `parsed`
  std::copy(offset, offset + rows + 1, s.h_off);
  if (rows) std::copy(label, label + rows, s.h_lab);
  for (int64_t r = 0; r < rows; ++r) {  // the row flags: a value that is not 1.0f
    uint8_t fl = 0;
    for (uint64_t k = offset[r]; k < offset[r + 1] && !fl; ++k) fl = value[k] != 1.f;
    s.h_flag[r] = fl;
  }
  DFX_HIP(hipMemcpyAsync(s.csr.off, s.h_off, (size_t)(rows + 1) * 8, hipMemcpyHostToDevice, up));
  if (nnz) DFX_HIP(hipMemcpyAsync(s.csr.idx, index, (size_t)nnz * 8, hipMemcpyHostToDevice, up));
  if (nnz)
    DFX_HIP(hipMemcpyAsync(s.csr.val, value, (size_t)nnz * 4, hipMemcpyHostToDevice, up));
  if (rows) {
    DFX_HIP(hipMemcpyAsync(s.csr.lab, s.h_lab, (size_t)rows * 4, hipMemcpyHostToDevice, up));
    DFX_HIP(hipMemcpyAsync(s.csr.flag, s.h_flag, (size_t)rows, hipMemcpyHostToDevice, up));
  }
  DFX_HIP(hipEventRecord(s.parsed, up));
  s.rows = rows;
  s.nnz = nnz;
  return DFX_OK;
}

extern "C" int dfx_textfeed_gather_valued(dfx_textfeed* f, int src, int to_batch,
                                          const uint32_t* rows, int64_t begin, int64_t n,
                                          int64_t r0, int64_t nnz) {
  DFX_CHECK_ARG(f && src >= -1 && src < (int)f->slot.size() && n >= 0 && r0 >= 0 && begin >= 0 &&
                    nnz >= 0,
                "textfeed_gather_valued: bad argument");
  DFX_FEED_FMT(f, DFX_TEXT_LIBSVM, "textfeed_gather_valued");
  DFX_CHECK_ARG(!to_batch || f->cur >= 0, "textfeed_gather_valued: no batch begun");
  DFX_CHECK_ARG(src >= 0 || to_batch, "textfeed_gather_valued: the shuffle buffer onto itself");
  if (n == 0) return DFX_OK;
  DFX_HIP(hipSetDevice(f->ctx->c.device));
  const DevCsr& S = src >= 0 ? f->slot[src].csr : f->shuf;
  DevCsr& D = to_batch ? f->ring[f->cur].csr : f->shuf;
  int64_t& used = to_batch ? f->ring[f->cur].nnz : f->shuf_nnz;
  DFX_CHECK_ARG(r0 + n <= D.cap, "textfeed_gather_valued: more rows than the destination holds");
  if (r0 == 0) used = 0;
  // the copies of a growth run on the gathers' stream: behind the gathers that filled the old
  // arrays and, for the shuffle buffer, behind the gathers that read them
  DFX_TRY(D.ensure_valued(D.cap, used + nnz, f->stream, r0, used));
  used += nnz;
  const uint32_t* rows_dev = nullptr;
  if (rows) {
    DFX_CHECK_ARG(to_batch, "textfeed_gather_valued: row lists go to the batch");
    auto& r = f->ring[f->cur];
    DFX_CHECK_ARG(r.used + n <= f->batch_rows,
                  "textfeed_gather_valued: row lists past the batch size");
    std::copy(rows, rows + n, r.h_rows + r.used);
    DFX_HIP(hipMemcpyAsync(r.d_rows + r.used, r.h_rows + r.used, (size_t)n * 4,
                           hipMemcpyHostToDevice, f->stream));
    rows_dev = r.d_rows + r.used;
    r.used += n;
  }
  if (src >= 0) DFX_HIP(hipStreamWaitEvent(f->stream, f->slot[src].parsed, 0));
  DFX_TRY(gather_rows_on<true>(&f->ctx->c, f->stream, S.off, S.idx, S.lab, rows_dev, begin, n,
                               D.off, D.idx, D.lab, r0, S.val, D.val, S.flag, D.flag));
  if (src >= 0) DFX_HIP(hipEventRecord(f->slot[src].gathered, f->stream));
  return DFX_OK;
}

extern "C" int dfx_textfeed_batch_end_valued(dfx_textfeed* f, int64_t rows, int64_t nnz,
                                             int valued, dfx_batch* out) {
  DFX_TRY(dfx_textfeed_batch_end(f, rows, nnz, out));
  DFX_FEED_FMT(f, DFX_TEXT_LIBSVM, "textfeed_batch_end_valued");
  out->value = valued ? f->ring[f->cur].csr.val : nullptr;
  return DFX_OK;
}

extern "C" int dfx_textfeed_slot_batch_valued(dfx_textfeed* f, int slot, int valued,
                                              dfx_batch* out) {
  DFX_TRY(dfx_textfeed_slot_batch(f, slot, out));
  DFX_FEED_FMT(f, DFX_TEXT_LIBSVM, "textfeed_slot_batch_valued");
  out->value = valued ? f->slot[slot].csr.val : nullptr;
  return DFX_OK;
}
