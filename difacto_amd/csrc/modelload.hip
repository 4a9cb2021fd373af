// A model file loaded on the device: SGDUpdater::Save's records (csrc/modeltext.h) cut apart,
// validated and inserted by kernels, with the effect of csrc/store.hip's dfx_store_load_part.
//
// Behind the aux byte the file is a run of dwords: a record is l1 = 4 + 2 aux of them (key, key,
// size, w [, sqrt_g, z]) or l2 = l1 + d (1 + aux) (then V [, Vaux]), told apart by its size
// dword, so a record's start depends on every size before it.  The whole file sits in one
// device buffer with the aux byte cut off (file byte 1 at the buffer's first, 256-byte aligned
// byte: every field a naturally aligned dword) and is cut into records in parallel:
//
//   k_ml_tilemap  a block per tile of tile_dwords dwords, staged in LDS with a 3-dword halo.
//                 Lane c walks the chain of records that enters the tile c dwords in (c in
//                 [0, l2): every phase a record of the tile before can hang over by) and leaves
//                 per (tile, c) where the chain leaves the tile - its overhang into the next, or
//                 why it ended - and its records, owned records and owned records with V.  An
//                 entry at or past the tile's end (a tile shorter than a record) leaves
//                 entry - tile_dwords and no counts.  A float payload whose bits look like a
//                 size keeps a false chain alive; only the chain from phase 0 of tile 0 is used.
//   k_ml_group    the scan whose operator composes these maps, level 1: a block per group of
//                 kMlGroup tiles, a lane per entry phase, -> the group's map
//   k_ml_top      level 2: one thread follows the group maps from phase 0 -> each group's entry
//                 and count prefixes, the totals and the verdict
//   k_ml_expand   a thread per group follows its tiles again -> each tile's entry and prefixes
//   k_ml_insert   a block per tile: lane 0 walks the true chain from the tile's entry and lists
//                 the record starts in LDS; the records are then spread over the lanes: the
//                 owner test, the V row's rank in file order (a block scan), tbl_insert and
//                 k_load's state rule by one lane, and V / Vaux copied out of the file buffer by
//                 consecutive lanes
//
// Nothing spins or looks back; no thread follows the file's tiles one by one (the longest
// dependent chains are kMlGroup loads, the groups, kMlGroup loads).  A chain ends as the host
// loader's loop ends, in its order: under 8 bytes left is the end of the file; a head or a V row
// cut short is `truncated model file`; a size above 1 that is not d + 1 is `model V_dim
// mismatch`; the key ~0 of a whole record is refused.  A size at or under 1 is a record without
// V, as `if (size > 1)` has it there.  The first of these in file order is the verdict, read
// back with the totals in the load's one wait; nothing is inserted before it.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <string>

#include "textscan.h"

namespace {

static_assert(kNT == kCountNT, "k_ml_insert's blocks go through block_count_add");
constexpr int kMlGroup = 128;                      // tiles composed by one level-1 block
constexpr int64_t kMlMinTile = 32, kMlMaxTile = 8192;  // tile_dwords: a multiple of 16 in between
constexpr int64_t kMlChunk = (int64_t)32 << 20;     // bytes of one pinned staging buffer, at most
constexpr int64_t kMlSlack = (int64_t)64 << 20;     // device memory left alone by the fit checks
// how a chain leaves a tile: its overhang (< kMlEnd), or why it ended
constexpr uint32_t kMlEnd = 0xFFF0u;       // under 8 bytes left: the host loop's clean end
constexpr uint32_t kMlTrunc = 0xFFF1u;
constexpr uint32_t kMlMismatch = 0xFFF2u;
constexpr uint32_t kMlBadKey = 0xFFF3u;

struct MlFile {
  const uint32_t* F;  // the file behind its aux byte
  int64_t nbytes;     // of it
  int64_t ndw;        // dwords that hold them (the last may be partial)
  int tile;           // tile_dwords
  int d, aux, l1, l2;
  int rank, nranks;
};

__device__ inline bool ml_owned(const MlFile& f, uint64_t key) {
  return (int)__umul64hi(key, (uint64_t)f.nranks) == f.rank;
}

// the record at dword pos of a tile staged in s (global dword gp) -> its dwords, or the reason
// the chain ends here (>= kMlEnd); *key, *has_v: of a whole record
__device__ inline uint32_t ml_record(const MlFile& f, const uint32_t* s, int pos, int64_t gp,
                                     uint64_t* key, bool* has_v) {
  const int64_t rem = f.nbytes - 4 * gp;
  if (rem < 8) return kMlEnd;
  if (rem < 4 * (int64_t)f.l1) return kMlTrunc;
  const int size = (int)s[pos + 2];
  *has_v = size > 1;
  if (size > 1) {
    if (size != f.d + 1) return kMlMismatch;
    if (rem < 4 * (int64_t)f.l2) return kMlTrunc;
  }
  *key = (uint64_t)s[pos] | ((uint64_t)s[pos + 1] << 32);
  if (*key == kEmptyKey) return kMlBadKey;
  return (uint32_t)(size > 1 ? f.l2 : f.l1);
}

// tile t and its halo into s[0, tile + 3)
__device__ inline void ml_stage(const MlFile& f, int64_t t, uint32_t* s) {
  const int64_t g0 = t * f.tile;
  for (int i = threadIdx.x; i < f.tile + 3; i += kNT) s[i] = g0 + i < f.ndw ? f.F[g0 + i] : 0u;
  __syncthreads();
}

// map[tile * l2 + c] = {exit | records << 16, owned | owned with V << 16}
__global__ __launch_bounds__(kNT) void k_ml_tilemap(MlFile f, int64_t tile0, uint2* map) {
  extern __shared__ uint32_t ml_lds[];
  const int64_t t = tile0 + blockIdx.x;
  ml_stage(f, t, ml_lds);
  for (int c = threadIdx.x; c < f.l2; c += kNT) {
    int pos = c;
    uint32_t nrec = 0, nown = 0, nownv = 0, exit;
    for (;;) {
      if (pos >= f.tile) { exit = (uint32_t)(pos - f.tile); break; }
      uint64_t key;
      bool has_v;
      const uint32_t len = ml_record(f, ml_lds, pos, t * f.tile + pos, &key, &has_v);
      if (len >= kMlEnd) { exit = len; break; }
      const bool own = ml_owned(f, key);
      ++nrec;
      nown += own;
      nownv += own && has_v;
      pos += (int)len;
    }
    map[t * f.l2 + c] = make_uint2(exit | (nrec << 16), nown | (nownv << 16));
  }
}

// state: a chain's phase at a tile's start, or how it ended; follows it through tiles [t0, t1)
struct MlWalk {
  uint32_t state, nrec, nown, nownv;
  __device__ void tile(const uint2* map, int64_t t, int l2) {
    const uint2 e = map[t * l2 + state];
    state = e.x & 0xFFFFu;
    nrec += e.x >> 16;
    nown += e.y & 0xFFFFu;
    nownv += e.y >> 16;
  }
};

__global__ __launch_bounds__(kNT) void k_ml_group(const uint2* __restrict__ map, int64_t ntiles,
                                                  int l2, uint4* __restrict__ gmap) {
  const int64_t t0 = (int64_t)blockIdx.x * kMlGroup, t1 = min(t0 + kMlGroup, ntiles);
  for (int c = threadIdx.x; c < l2; c += kNT) {
    MlWalk w{(uint32_t)c, 0, 0, 0};
    for (int64_t t = t0; t < t1 && w.state < kMlEnd; ++t) w.tile(map, t, l2);
    gmap[(int64_t)blockIdx.x * l2 + c] = make_uint4(w.state, w.nrec, w.nown, w.nownv);
  }
}

// gent[g] = {the true chain's state at group g's start, owned before it, owned with V before it}
// res = {verdict, records, owned, owned with V}
__global__ void k_ml_top(const uint4* __restrict__ gmap, int64_t ngroups, int l2,
                         uint4* __restrict__ gent, unsigned long long* res) {
  if (blockIdx.x || threadIdx.x) return;
  MlWalk w{0, 0, 0, 0};
  for (int64_t g = 0; g < ngroups; ++g) {
    gent[g] = make_uint4(w.state, w.nown, w.nownv, 0);
    if (w.state >= kMlEnd) continue;
    const uint4 e = gmap[g * l2 + w.state];
    w.state = e.x;
    w.nrec += e.y;
    w.nown += e.z;
    w.nownv += e.w;
  }
  // (a whole record never passes the file's end, so a chain that is still alive stands on it)
  res[0] = w.state == kMlEnd || w.state == 0 ? 0 : w.state < kMlEnd ? kMlTrunc : w.state;
  res[1] = w.nrec;
  res[2] = w.nown;
  res[3] = w.nownv;
}

__global__ __launch_bounds__(kWave) void k_ml_expand(const uint2* __restrict__ map,
                                                     int64_t ntiles, int64_t ngroups, int l2,
                                                     const uint4* __restrict__ gent,
                                                     uint4* __restrict__ tent) {
  const int64_t g = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (g >= ngroups) return;
  const uint4 e = gent[g];
  MlWalk w{e.x, 0, e.y, e.z};
  const int64_t t0 = g * kMlGroup, t1 = min(t0 + kMlGroup, ntiles);
  for (int64_t t = t0; t < t1; ++t) {
    tent[t] = make_uint4(w.state, w.nown, w.nownv, 0);
    if (w.state < kMlEnd) w.tile(map, t, l2);
  }
}

// dynamic LDS: the staged tile, the tile's record starts (bit 31: has V), their V rows (-1: none
// to copy), the block scan
__host__ __device__ inline int ml_max_records(int tile) { return tile / 4 + 1; }
size_t ml_insert_lds(int tile) {
  return sizeof(uint32_t) * ((size_t)tile + 4 + 2 * (size_t)ml_max_records(tile) + 2 * kNT);
}

__global__ __launch_bounds__(kNT) void k_ml_insert(MlFile f, const uint4* __restrict__ tent,
                                                   Table T, DevState* ds, int64_t nv0) {
  extern __shared__ uint32_t ml_lds[];
  __shared__ uint32_t s_n;
  const int64_t t = blockIdx.x;
  const uint4 ent = tent[t];
  if (ent.x >= kMlEnd) return;  // (the whole block: the true chain ended before this tile)
  uint32_t* stage = ml_lds;
  uint32_t* start = stage + f.tile + 4;
  int32_t* vrow = reinterpret_cast<int32_t*>(start + ml_max_records(f.tile));
  uint32_t* scan = reinterpret_cast<uint32_t*>(vrow + ml_max_records(f.tile));
  ml_stage(f, t, stage);
  const int64_t g0 = t * f.tile;
  if (threadIdx.x == 0) {
    uint32_t n = 0;
    for (int pos = (int)ent.x; pos < f.tile;) {
      uint64_t key;
      bool has_v;
      const uint32_t len = ml_record(f, stage, pos, g0 + pos, &key, &has_v);
      if (len >= kMlEnd) break;  // (the file's end: the verdict was OK)
      start[n++] = (uint32_t)pos | (has_v ? 0x80000000u : 0u);
      pos += (int)len;
    }
    s_n = n;
  }
  __syncthreads();
  const uint32_t n = s_n;
  int ins = 0;
  uint32_t vbase = ent.z;  // owned records with V in front of round r0, in file order
  for (uint32_t r0 = 0; r0 < n; r0 += kNT) {
    const uint32_t r = r0 + threadIdx.x;
    int pos = 0;
    bool has_v = false, own = false;
    uint64_t key = 0;
    if (r < n) {
      pos = (int)(start[r] & 0x7FFFFFFFu);
      has_v = start[r] >> 31;
      key = (uint64_t)stage[pos] | ((uint64_t)stage[pos + 1] << 32);
      own = ml_owned(f, key);
    }
    uint32_t incl, excl, total;
    block_scan<AddOp, kNT>(own && has_v ? 1u : 0u, scan, &incl, &excl, &total);
    if (r < n) {
      int32_t row = -1;
      if (own) {
        bool inserted;
        const int64_t s = tbl_insert(T, key, &inserted);
        ins += inserted;
        if (s < 0) {
          atomicOr(&ds->err, insert_error(s));
        } else {  // k_load's rule: fea_cnt kept, sqrt_g / z kept when the file has no aux
          Entry* en = ent_at(T, s);
          const uint32_t* rec = f.F + g0 + pos;
          float4 e = ent_state(en);
          e.x = __uint_as_float(rec[3]);
          if (f.aux) {
            e.y = __uint_as_float(rec[4]);
            e.z = __uint_as_float(rec[5]);
          }
          ent_set_state(en, e);
          if (has_v) {
            row = T.es ? (int32_t)s : (int32_t)(nv0 + vbase + excl);
            en->vrow = row;
          }
        }
      }
      vrow[r] = row;
    }
    vbase += total;
  }
  __syncthreads();
  // V and Vaux: a group of G consecutive lanes per record, a dword per lane and round
  const int G = next_pow2_lanes(f.d), d = f.d;
  for (uint32_t r = threadIdx.x / G; r < n; r += kNT / G) {
    const int32_t row = vrow[r];
    if (row < 0) continue;
    const uint32_t* src = f.F + g0 + (start[r] & 0x7FFFFFFFu) + (f.aux ? 6 : 4);
    float* V = row_V(T, row);
    for (int k = threadIdx.x % G; k < d; k += G) {
      V[k] = __uint_as_float(src[k]);
      vaux_put(T, row, k, f.aux ? __uint_as_float(src[d + k]) : 0.f);
    }
  }
  block_count_add(ins, &ds->n_keys);
}

// n_vrows past the loaded rows; new_w = model_.size() (sgd_updater.h:91)
__global__ void k_ml_finish(DevState* ds, unsigned long long n_vrows) {
  ds->n_vrows = n_vrows;
  ds->new_w = (long long)ds->n_keys;
}

// ---- the host side --------------------------------------------------------------------------
struct MlHeld {  // what one load holds until it returns
  FILE* f = nullptr;
  void* dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~MlHeld() { release(); }
  void release() {
    if (f) fclose(f);
    f = nullptr;
    for (void*& p : dev) {
      if (p) (void)hipFree(p);
      p = nullptr;
    }
  }
};

double ml_now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

int ml_staging_reserve(MlStaging& S, int64_t bytes) {
  if (!S.res) {
    DFX_HIP(hipHostMalloc(reinterpret_cast<void**>(&S.res), 4 * sizeof(unsigned long long),
                          hipHostMallocDefault));
    for (int k = 0; k < 2; ++k) DFX_HIP(hipEventCreateWithFlags(&S.ev[k], hipEventDisableTiming));
  }
  if (bytes <= S.cap_bytes) return DFX_OK;
  for (int k = 0; k < 2; ++k) {
    if (S.host[k]) (void)hipHostFree(S.host[k]);
    S.host[k] = nullptr;
  }
  S.cap_bytes = 0;
  for (int k = 0; k < 2; ++k)
    DFX_HIP(hipHostMalloc(reinterpret_cast<void**>(&S.host[k]), (size_t)bytes,
                          hipHostMallocDefault));
  S.cap_bytes = bytes;
  return DFX_OK;
}

// the host loader in the device's place
int ml_host(dfx_ctx* ctx, const char* path, int rank, int nranks, MlHeld& H, int64_t* stats) {
  H.release();
  if (stats) stats[5] = 1;
  return dfx_store_load_part(ctx, path, rank, nranks);
}

int ml_load(dfx_ctx* ctx, const char* path, int rank, int nranks, int64_t tile_dwords,
            int64_t* stats, double* times) {
  DFX_CHECK_ARG(ctx && path, "null argument");
  DFX_CHECK_ARG(nranks >= 1 && rank >= 0 && rank < nranks, "store_load_dev: bad rank");
  DFX_CHECK_ARG(tile_dwords == 0 || (tile_dwords >= kMlMinTile && tile_dwords <= kMlMaxTile &&
                                     tile_dwords % 16 == 0),
                "store_load_dev: tile_dwords must be 0 or a multiple of 16 in [32, 8192]");
  Context* c = &ctx->c;
  DFX_CHECK_ARG(!c->vrows_half && c->slot_line != 3, "vrows=f16: the device model loader writes fp32 pool rows; use the "
                            "host loader (dfx_store_load, model_read=host)");
  DFX_HIP(hipSetDevice(c->device));
  if (stats) std::fill(stats, stats + 6, (int64_t)0);
  if (times) times[0] = times[1] = 0;
  DFX_TRY(table_set_ranges(c, nranks));
  MlHeld H;
  H.f = fopen(path, "rb");
  if (!H.f) { set_error(std::string("cannot open ") + path); return DFX_ERR_IO; }
  bool aux_byte;
  if (fread(&aux_byte, sizeof(bool), 1, H.f) != 1) return DFX_OK;
  if (fseeko(H.f, 0, SEEK_END) != 0) { set_error(std::string("cannot seek ") + path); return DFX_ERR_IO; }
  const int64_t nbytes = (int64_t)ftello(H.f) - 1;
  if (fseeko(H.f, 1, SEEK_SET) != 0) { set_error(std::string("cannot seek ") + path); return DFX_ERR_IO; }

  MlFile f{};
  f.d = c->T.d;
  f.aux = aux_byte ? 1 : 0;
  f.l1 = 4 + 2 * f.aux;
  f.l2 = f.l1 + f.d * (1 + f.aux);
  f.rank = rank;
  f.nranks = nranks;
  f.nbytes = nbytes;
  f.ndw = (nbytes + 3) / 4;
  // a long record's map rows cost 8 l2 bytes a tile: wider tiles keep them a small share
  f.tile = (int)(tile_dwords ? tile_dwords : f.l2 <= 128 ? 4096 : kMlMaxTile);
  const int64_t ntiles = (f.ndw + f.tile - 1) / f.tile;
  const int64_t ngroups = (ntiles + kMlGroup - 1) / kMlGroup;
  if (stats) {
    stats[3] = ntiles;
    stats[4] = f.tile;
  }
  const hipStream_t st = c->stream;
  DFX_HIP(hipStreamSynchronize(st));
  unsigned long long res[4] = {0, 0, 0, 0};
  double read_s = 0, wait_s = 0;
  uint4* tent = nullptr;
  if (ntiles > 0) {
    // what the maps pack into 16 bits, and the 32-bit prefixes
    if (f.l2 >= (int)kMlEnd || nbytes / 16 >= ((int64_t)1 << 31))
      return ml_host(ctx, path, rank, nranks, H, stats);
    const size_t sizes[5] = {(size_t)f.ndw * 4 + 16, (size_t)ntiles * f.l2 * sizeof(uint2),
                             (size_t)ngroups * f.l2 * sizeof(uint4),
                             ((size_t)ngroups + 2) * sizeof(uint4),
                             (size_t)ntiles * sizeof(uint4)};
    size_t need = 0, free_b = 0, total_b = 0;
    for (size_t s : sizes) need += s + 256;
    DFX_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need + (size_t)kMlSlack > free_b) return ml_host(ctx, path, rank, nranks, H, stats);
    for (int i = 0; i < 5; ++i) DFX_HIP(hipMalloc(&H.dev[i], sizes[i]));
    char* F = static_cast<char*>(H.dev[0]);
    uint2* map = static_cast<uint2*>(H.dev[1]);
    uint4* gmap = static_cast<uint4*>(H.dev[2]);
    uint4* gent = static_cast<uint4*>(H.dev[3]);
    tent = static_cast<uint4*>(H.dev[4]);
    f.F = reinterpret_cast<const uint32_t*>(F);
    MlStaging& S = c->ml_stage;
    const int64_t chunk = std::min(kMlChunk, (nbytes + 0xFFFFF) & ~(int64_t)0xFFFFF);
    DFX_TRY(ml_staging_reserve(S, chunk));
    const size_t lds = sizeof(uint32_t) * ((size_t)f.tile + 4);
    int64_t tiles_done = 0;
    // chunk t is read while chunk t - 1 is copied and its tiles are mapped; a tile is mapped
    // once its halo has arrived
    for (int64_t off = 0, t = 0; off < nbytes; off += chunk, ++t) {
      const int k = (int)(t & 1);
      const int64_t nb = std::min(chunk, nbytes - off);
      double t0 = ml_now();
      if (t >= 2) DFX_HIP(hipEventSynchronize(S.ev[k]));  // its last copy has left the buffer
      wait_s += ml_now() - t0;
      t0 = ml_now();
      if ((int64_t)fread(S.host[k], 1, (size_t)nb, H.f) != nb) {
        set_error(std::string("short read of ") + path);
        return DFX_ERR_IO;
      }
      read_s += ml_now() - t0;
      DFX_HIP(hipMemcpyAsync(F + off, S.host[k], (size_t)nb, hipMemcpyHostToDevice, st));
      DFX_HIP(hipEventRecord(S.ev[k], st));
      const int64_t have = (off + nb) / 4;  // whole dwords on the device
      const int64_t ready = off + nb == nbytes ? ntiles : std::max<int64_t>(have - 3, 0) / f.tile;
      if (ready > tiles_done) {
        hipLaunchKernelGGL(k_ml_tilemap, dim3((unsigned)(ready - tiles_done)), dim3(kNT), lds, st,
                           f, tiles_done, map);
        tiles_done = ready;
      }
    }
    hipLaunchKernelGGL(k_ml_group, dim3((unsigned)ngroups), dim3(kNT), 0, st,
                       (const uint2*)map, ntiles, f.l2, gmap);
    unsigned long long* res_dev = reinterpret_cast<unsigned long long*>(gent + ngroups);
    hipLaunchKernelGGL(k_ml_top, dim3(1), dim3(kWave), 0, st, (const uint4*)gmap, ngroups, f.l2,
                       gent, res_dev);
    hipLaunchKernelGGL(k_ml_expand, dim3(blocks_for((uint64_t)ngroups, kWave)), dim3(kWave), 0,
                       st, (const uint2*)map, ntiles, ngroups, f.l2, (const uint4*)gent, tent);
    DFX_HIP(hipGetLastError());
    DFX_HIP(hipMemcpyAsync(S.res, res_dev, sizeof(res), hipMemcpyDeviceToHost, st));
    const double t0 = ml_now();
    DFX_HIP(hipStreamSynchronize(st));  // the load's one wait: the totals and the verdict
    wait_s += ml_now() - t0;
    std::copy(S.res, S.res + 4, res);
  }
  if (times) {
    times[0] = read_s;
    times[1] = wait_s;
  }
  if (res[0] == kMlMismatch) { set_error("model V_dim mismatch"); return DFX_ERR_CHECK; }
  if (res[0] == kMlBadKey) {
    set_error("model file holds key 0xffffffffffffffff, reserved as the empty-slot marker");
    return DFX_ERR_ARG;
  }
  if (res[0] != 0) { set_error("truncated model file"); return DFX_ERR_IO; }
  const int64_t nrec = (int64_t)res[1], nown = (int64_t)res[2], nownv = (int64_t)res[3];
  if (stats) {
    stats[0] = nrec;
    stats[1] = nown;
    stats[2] = nownv;
  }
  int64_t n_keys = 0, n_vrows = 0;
  DFX_TRY(dfx_store_stats(ctx, &n_keys, &n_vrows, nullptr, nullptr));
  {  // the table store_reserve will build has to fit beside the file
    const int64_t grow = store_reserve_bytes(c, n_keys + nown, n_vrows + nownv);
    size_t free_b = 0, total_b = 0;
    DFX_HIP(hipMemGetInfo(&free_b, &total_b));
    if (grow > 0 && (size_t)(grow + kMlSlack) > free_b)
      return ml_host(ctx, path, rank, nranks, H, stats);
  }
  DFX_TRY(store_reserve(c, n_keys + nown, n_vrows + nownv));
  if (nown == 0) return DFX_OK;
  hipLaunchKernelGGL(k_ml_insert, dim3((unsigned)ntiles), dim3(kNT), ml_insert_lds(f.tile), st, f,
                     (const uint4*)tent, c->T, c->ds, n_vrows);
  hipLaunchKernelGGL(k_ml_finish, dim3(1), dim3(1), 0, st, c->ds,
                     (unsigned long long)(n_vrows + nownv));
  DFX_HIP(hipGetLastError());
  return dfx_sync(ctx);  // (the file buffer is freed behind it)
}

}  // namespace

extern "C" int dfx_store_load_dev(dfx_ctx* ctx, const char* path, int rank, int nranks,
                                  int64_t tile_dwords, int64_t* stats, double* times) {
  const int rc = ml_load(ctx, path, rank, nranks, tile_dwords, stats, times);
  // (a failed call may leave copies queued that read the context's staging buffers: join them)
  if (rc != DFX_OK && ctx) (void)hipStreamSynchronize(ctx->c.stream);
  return rc;
}
