// Criteo text -> CSR on the device, and the device form of the host reader's row gather.
//
//   dfx_parse_criteo   ParseCriteo (difacto_amd/host/reader.cc; criteo_parser.h:40-92) over a
//                      chunk of whole lines already in device memory
//   dfx_gather_rows    GatherRows (reader.cc; the row copies of batch_reader.cc:29-78);
//                      dfx_gather_rows_valued: the same kernels with values and row flags
// The scans (block_scan, k_scan_*) are csrc/textscan.h, shared with libsvmparse.hip; the text
// feed that runs the parsers and the gather beside the step is textfeed.hip.
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

}  // namespace

template <bool kValued>
int dfx::gather_rows_on(Context* c, hipStream_t st, const uint64_t* src_offset,
                        const uint64_t* src_index, const float* src_label,
                        const uint32_t* rows_dev, int64_t begin, int64_t n, uint64_t* dst_offset,
                        uint64_t* dst_index, float* dst_label, int64_t r0, const float* src_value,
                        float* dst_value, const uint8_t* src_flag, uint8_t* dst_flag) {
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

// the feed (textfeed.hip) picks one of the two by its format
#define DFX_GATHER_ROWS_ON(kValued)                                                              \
  template int dfx::gather_rows_on<kValued>(                                                     \
      Context*, hipStream_t, const uint64_t*, const uint64_t*, const float*, const uint32_t*,    \
      int64_t, int64_t, uint64_t*, uint64_t*, float*, int64_t, const float*, float*,             \
      const uint8_t*, uint8_t*)
DFX_GATHER_ROWS_ON(false);
DFX_GATHER_ROWS_ON(true);
#undef DFX_GATHER_ROWS_ON

int dfx::parse_criteo_on(const TpScratch& ws, hipStream_t st, const char* text, int64_t nbytes,
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

int dfx::capacity_status(const int64_t* stat) {
  if (!stat[3]) return DFX_OK;
  set_error("parse_criteo: the chunk needs " + std::to_string(stat[0]) + " rows and " +
            std::to_string(stat[1]) + " ids, more than the caller's capacity");
  return DFX_ERR_CAPACITY;
}

extern "C" int dfx_parse_criteo(dfx_ctx* ctx, const char* text_dev, int64_t nbytes, int is_train,
                                int64_t max_rows, int64_t max_nnz, uint64_t* offset,
                                uint64_t* index, float* label, int64_t* stat_dev) {
  DFX_CHECK_ARG(ctx, "null ctx");
  DFX_HIP(hipSetDevice(ctx->c.device));
  Context* c = &ctx->c;
  return parse_criteo_on(context_scratch(c), input_stream(c), text_dev, nbytes, is_train,
                         max_rows, max_nnz, offset, index, label, stat_dev);
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
