// The device reshuffler: a fresh shuffle of a cached part in every epoch.  The batch cache
// (batchcache.hip) replays the reader's batches as recorded, the same rows in the same batches
// in every epoch; the reference's reader draws from a rand() state that is never reseeded
// (src/reader/batch_reader.cc:38-45), so its epochs see other batch compositions.  The rows are
// already in device memory: a reshuffled epoch is a row gather over the whole sealed list, the
// N rows of its batches in order, through a keyed bijection of [0, N) computed per row
// (reshuffle.h: no permutation array, no sort, no host list), cut every batch_rows rows.
//
// Per epoch (dfx_reshuffle_begin_epoch), on the context's input stream:
//   k_rs_len    per output position j its source row rs_apply(net, j), found in the batches'
//               row prefix by bisection, and that row's length
//   k_rs_scan   one block per output batch scans its segment [k R, (k + 1) R) of the lengths:
//               every row's exclusive offset inside its batch, and the batch's nnz into a
//               pinned host array
// and ONE host wait for those nnz (dfx_batch.nnz is a host value), never one per batch.
// Per batch (dfx_reshuffle_next): the input stream waits for the ring entry's `consumed` event
// (a stream wait, the host never blocks) and one k_rs_copy launch, a wave per row, recomputes
// each row's source and moves its ids, values (ones for a binary source), label and weight (1
// where the source has none) and writes the rebased offsets.  The sources are only read.
//
// A sampled epoch (dfx_reshuffle_begin_epoch_sampled) is the same epoch without the negative
// rows a keyed draw per SOURCE row drops (reshuffle.h: rs_dropped, the reader's inequality): a
// fresh down-sample per epoch over a list that holds every row, where a reader's one sample
// would replay for ever.  k_rs_keep writes source, length and keep flag per position, a
// multi-launch scan of the flags (k_rs_tiles, k_rs_compact) compacts the kept rows' sources
// and lengths in permuted order, the per-batch scan runs over the K kept rows (k_rs_scan_k; K
// goes to the pinned array with the nnz, still one host wait), and the copy reads the
// compacted sources (k_rs_copy_k).  8 bytes a row more, taken at the first sampled epoch.
//
// Memory, all inside the cache's budget: a table of the batches' five pointers and their row
// prefix, 12 bytes a row of per-epoch scratch, and a ring of nring destination batches whose
// nnz capacity starts at 1.25 times the mean batch and is regrown, after the ring's `consumed`
// events, when an epoch's largest batch needs more.  What does not fit is reported (*kept = 0,
// n_batches = -1) and the caller replays the list as recorded; nothing fails.  A batch holds
// fewer than 2^32 ids, a list fewer than 2^31 rows.
#include <algorithm>
#include <vector>

#include "internal.h"
#include "reshuffle.h"

using namespace dfx;

namespace {
constexpr int64_t kAlign = 256;
constexpr int kNT = 256, kWavesPerBlock = kNT / kWave, kScanItems = 8;
inline int64_t round_up(int64_t n) { return (std::max<int64_t>(n, 1) + kAlign - 1) / kAlign * kAlign; }

struct RsSrc {  // a source batch's arrays (val, wt: NULL when the batch has none)
  const uint64_t* off;
  const uint64_t* idx;
  const float* val;
  const float* lab;
  const float* wt;
};
struct RsDst {  // a ring entry's arrays (val, wt: NULL when no batch of the list has them)
  uint64_t* off;
  uint64_t* idx;
  float* val;
  float* lab;
  float* wt;
};

// the batch b of list row p: prefix[b] <= p < prefix[b + 1] (prefix[0] = 0, prefix[nb] = N > p;
// an empty batch has equal neighbours and is never the answer)
__device__ inline uint32_t rs_find(const uint32_t* __restrict__ prefix, uint32_t nb, uint32_t p) {
  uint32_t lo = 0, hi = nb;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (prefix[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kNT) void k_rs_len(rs_net net, const RsSrc* __restrict__ src,
                                                const uint32_t* __restrict__ prefix, uint32_t nb,
                                                uint32_t* __restrict__ len) {
  const uint64_t j64 = (uint64_t)blockIdx.x * kNT + threadIdx.x;
  if (j64 >= net.n) return;
  const uint32_t p = rs_apply(net, (uint32_t)j64);
  const uint32_t b = rs_find(prefix, nb, p);
  const uint32_t r = p - prefix[b];
  const uint64_t* off = src[b].off;
  len[j64] = (uint32_t)(off[r + 1] - off[r]);
}

// block k: rows [k R, min((k + 1) R, n)) of len -> their exclusive offsets, the sum to bnnz[k]
// (pinned host memory)
__device__ inline void rs_scan_block(const uint32_t* __restrict__ len, uint32_t n, uint32_t R,
                                     uint64_t* __restrict__ ex,
                                     unsigned long long* __restrict__ bnnz, uint32_t* lds) {
  const uint64_t lo = (uint64_t)blockIdx.x * R;
  const uint64_t hi = lo + R < n ? lo + R : n;
  uint64_t carry = 0;
  // kScanItems consecutive rows a thread: a batch of 100,000 rows is 49 rounds of the block
  for (uint64_t t = lo; t < hi; t += (uint64_t)kNT * kScanItems) {
    const uint64_t j = t + (uint64_t)threadIdx.x * kScanItems;
    uint32_t v[kScanItems], sum = 0;
#pragma unroll
    for (int q = 0; q < kScanItems; ++q) {
      v[q] = j + q < hi ? len[j + q] : 0u;
      sum += v[q];
    }
    uint32_t total;
    uint64_t e = carry + block_excl_scan<kNT>(sum, lds, &total);
#pragma unroll
    for (int q = 0; q < kScanItems; ++q) {
      if (j + q < hi) ex[j + q] = e;
      e += v[q];
    }
    carry += total;
  }
  if (threadIdx.x == 0) bnnz[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kNT) void k_rs_scan(const uint32_t* __restrict__ len, uint32_t n,
                                                 uint32_t R, uint64_t* __restrict__ ex,
                                                 unsigned long long* __restrict__ bnnz) {
  __shared__ uint32_t lds[kNT / kWave + 1];
  rs_scan_block(len, n, R, ex, bnnz, lds);
}

// ---- a sampled epoch (dfx_reshuffle_begin_epoch_sampled) --------------------------------------
// Three launches compact the kept rows in permuted order; the order is a scan's, never a
// ticket's, so it does not depend on timing:
//   k_rs_keep     per output position j: its source row, that row's length and the keep flag
//                 (the flag in the source's top bit: a list holds fewer than 2^31 rows), and per
//                 tile of kTile positions the number kept
//   k_rs_tiles    one block: the tiles' exclusive prefix in place, the kept total K behind it
//   k_rs_compact  per tile: a block scan of its flags, the kept rows' source and length to
//                 ksrc[c], klen[c], c = the tile's prefix + the row's rank in the tile
// then k_rs_scan_k, k_rs_scan over klen[0, K) with K read from the device.
constexpr uint32_t kTile = kNT * kScanItems;
constexpr uint32_t kKeepBit = 0x80000000u;

__global__ __launch_bounds__(kNT) void k_rs_keep(rs_net net, uint64_t key, float neg_sampling,
                                                 const RsSrc* __restrict__ src,
                                                 const uint32_t* __restrict__ prefix, uint32_t nb,
                                                 uint32_t* __restrict__ len,
                                                 uint32_t* __restrict__ flagged,
                                                 uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t lds[kNT / kWave + 1];
  const uint64_t j0 = (uint64_t)blockIdx.x * kTile;
  uint32_t cnt = 0;
#pragma unroll 1
  for (int q = 0; q < kScanItems; ++q) {
    const uint64_t j64 = j0 + (uint64_t)q * kNT + threadIdx.x;
    if (j64 >= net.n) break;
    const uint32_t p = rs_apply(net, (uint32_t)j64);
    const uint32_t b = rs_find(prefix, nb, p);
    const uint32_t r = p - prefix[b];
    const uint64_t* off = src[b].off;
    const bool keep = !rs_dropped(key, p, src[b].lab[r], neg_sampling);
    len[j64] = (uint32_t)(off[r + 1] - off[r]);
    flagged[j64] = keep ? p | kKeepBit : p;
    cnt += keep ? 1u : 0u;
  }
  uint32_t total;
  (void)block_excl_scan<kNT>(cnt, lds, &total);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// tile[0, nt): counts -> exclusive prefix, in place; tile[nt] = the total, also to *hK (pinned)
__global__ __launch_bounds__(kNT) void k_rs_tiles(uint32_t* __restrict__ tile, uint32_t nt,
                                                  unsigned long long* __restrict__ hK) {
  __shared__ uint32_t lds[kNT / kWave + 1];
  uint32_t carry = 0;
  for (uint32_t t = 0; t < nt; t += kTile) {
    const uint64_t j = (uint64_t)t + (uint64_t)threadIdx.x * kScanItems;
    uint32_t v[kScanItems], sum = 0;
#pragma unroll
    for (int q = 0; q < kScanItems; ++q) {
      v[q] = j + q < nt ? tile[j + q] : 0u;
      sum += v[q];
    }
    uint32_t total;
    uint32_t e = carry + block_excl_scan<kNT>(sum, lds, &total);
#pragma unroll
    for (int q = 0; q < kScanItems; ++q) {
      if (j + q < nt) tile[j + q] = e;
      e += v[q];
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    tile[nt] = carry;
    *hK = carry;
  }
}

__global__ __launch_bounds__(kNT) void k_rs_compact(const uint32_t* __restrict__ flagged,
                                                    const uint32_t* __restrict__ len, uint32_t n,
                                                    const uint32_t* __restrict__ tile_pre,
                                                    uint32_t* __restrict__ ksrc,
                                                    uint32_t* __restrict__ klen) {
  __shared__ uint32_t lds[kNT / kWave + 1];
  const uint64_t j = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kScanItems;
  uint32_t f[kScanItems], cnt = 0;
#pragma unroll
  for (int q = 0; q < kScanItems; ++q) {
    f[q] = j + q < n ? flagged[j + q] : 0u;
    cnt += f[q] >> 31;
  }
  uint32_t c = tile_pre[blockIdx.x] + block_excl_scan<kNT>(cnt, lds, nullptr);
#pragma unroll
  for (int q = 0; q < kScanItems; ++q)
    if (f[q] & kKeepBit) {  // (a position at or past n reads as 0: not kept)
      ksrc[c] = f[q] & ~kKeepBit;
      klen[c] = len[j + q];
      ++c;
    }
}

// k_rs_scan over klen[0, *K): the grid is the N rows' (K is not on the host yet); a block at or
// past K writes an nnz of 0
__global__ __launch_bounds__(kNT) void k_rs_scan_k(const uint32_t* __restrict__ klen,
                                                   const uint32_t* __restrict__ K, uint32_t R,
                                                   uint64_t* __restrict__ ex,
                                                   unsigned long long* __restrict__ bnnz) {
  __shared__ uint32_t lds[kNT / kWave + 1];
  rs_scan_block(klen, *K, R, ex, bnnz, lds);
}

// the wave's row i of the output batch that starts at position j0: list row p into the ring entry
__device__ inline void rs_copy_row(const RsSrc* __restrict__ src,
                                   const uint32_t* __restrict__ prefix, uint32_t nb,
                                   const uint64_t* __restrict__ ex, uint32_t j0, uint32_t i,
                                   uint32_t p, uint32_t lane, const RsDst& d) {
  const uint32_t b = rs_find(prefix, nb, p);
  const uint32_t r = p - prefix[b];
  const RsSrc s = src[b];
  const uint64_t s0 = s.off[r], len = s.off[r + 1] - s0, d0 = ex[j0 + i];
  for (uint64_t k = lane; k < len; k += 64) d.idx[d0 + k] = s.idx[s0 + k];
  if (d.val) {
    if (s.val)
      for (uint64_t k = lane; k < len; k += 64) d.val[d0 + k] = s.val[s0 + k];
    else
      for (uint64_t k = lane; k < len; k += 64) d.val[d0 + k] = 1.f;
  }
  if (lane == 0) {
    d.off[i + 1] = d0 + len;
    d.lab[i] = s.lab[r];
    if (d.wt) d.wt[i] = s.wt ? s.wt[r] : 1.f;
    if (i == 0) d.off[0] = 0;
  }
}

// one wave per row i of the output batch that starts at list position j0
__global__ __launch_bounds__(kNT) void k_rs_copy(rs_net net, const RsSrc* __restrict__ src,
                                                 const uint32_t* __restrict__ prefix, uint32_t nb,
                                                 const uint64_t* __restrict__ ex, uint32_t j0,
                                                 uint32_t rows, RsDst d) {
  const uint64_t i64 = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (i64 >= rows) return;
  const uint32_t lane = threadIdx.x & 63;
  // (the same for the wave's lanes: the walk and the bisection run on the scalar unit)
  const uint32_t i = __builtin_amdgcn_readfirstlane((uint32_t)i64);
  rs_copy_row(src, prefix, nb, ex, j0, i, rs_apply(net, j0 + i), lane, d);
}

// ... of a sampled epoch: the row's source is read from ksrc, not recomputed
__global__ __launch_bounds__(kNT) void k_rs_copy_k(const uint32_t* __restrict__ ksrc,
                                                   const RsSrc* __restrict__ src,
                                                   const uint32_t* __restrict__ prefix,
                                                   uint32_t nb, const uint64_t* __restrict__ ex,
                                                   uint32_t j0, uint32_t rows, RsDst d) {
  const uint64_t i64 = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (i64 >= rows) return;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = __builtin_amdgcn_readfirstlane((uint32_t)i64);
  rs_copy_row(src, prefix, nb, ex, j0, i, __builtin_amdgcn_readfirstlane(ksrc[j0 + i]), lane, d);
}
}  // namespace

struct dfx_reshuffle {
  dfx_batchcache* bc = nullptr;
  dfx_ctx* ctx = nullptr;
  int64_t N = 0, R = 1, nb_src = 0, nb_out = 0, total_nnz = 0;
  bool valued = false, weighted = false;
  // the table and the per-epoch scratch: one device allocation
  void* scratch = nullptr;
  int64_t scratch_bytes = 0;
  RsSrc* d_src = nullptr;
  uint32_t *d_prefix = nullptr, *d_len = nullptr;
  uint64_t* d_ex = nullptr;
  std::vector<RsSrc> h_src;  // what the table's upload reads
  std::vector<uint32_t> h_prefix;
  // pinned: the epoch's nnz per output batch; [nb_out]: a sampled epoch's kept rows
  unsigned long long* h_bnnz = nullptr;
  hipEvent_t ev_epoch = nullptr;
  struct Entry {
    void* base = nullptr;
    int64_t bytes = 0;
    RsDst d{};
    hipEvent_t consumed = nullptr;
  };
  std::vector<Entry> ring;
  int64_t cap = 0;  // a ring entry's nnz capacity; 0: no ring (a growth did not fit)
  rs_net net{};
  // a sampled epoch's scratch, taken at the first dfx_reshuffle_begin_epoch_sampled: the kept
  // rows' sources and lengths, the tiles' prefix with the kept total behind it
  void* samp = nullptr;
  int64_t samp_bytes = 0;
  uint32_t *d_ksrc = nullptr, *d_klen = nullptr, *d_tile = nullptr;
  bool sampled = false;          // the open epoch is a sampled one
  int64_t n_cur = 0, nb_cur = 0; // the open epoch's rows and batches (N, nb_out when not sampled)
  bool epoch_open = false;
  int64_t pos = 0;
  int handed = -1;  // the ring entry of the batch handed out and not yet marked consumed
};

namespace {
inline hipStream_t in_stream(dfx_reshuffle* rs) {
  const Context& c = rs->ctx->c;
  return c.has_in_stream ? c.in_stream : c.stream;
}

void ring_free(dfx_reshuffle* rs) {
  for (auto& e : rs->ring) {
    if (e.base) batchcache_give(rs->bc, e.base, e.bytes);
    e.base = nullptr;
    e.bytes = 0;
    e.d = RsDst{};
  }
  rs->cap = 0;
}

// every ring entry with room for cap ids -> 1; over the budget or out of memory -> 0 (no ring
// left); another HIP failure -> -1
int ring_alloc(dfx_reshuffle* rs, int64_t cap) {
  const int64_t R = rs->R;
  const int64_t part[5] = {round_up((R + 1) * 8), round_up(cap * 8),
                           rs->valued ? round_up(cap * 4) : 0, round_up(R * 4),
                           rs->weighted ? round_up(R * 4) : 0};
  const int64_t bytes = part[0] + part[1] + part[2] + part[3] + part[4];
  for (auto& e : rs->ring) {
    void* p = nullptr;
    const int rc = batchcache_take(rs->bc, bytes, &p);
    if (rc != 1) {
      ring_free(rs);
      return rc;
    }
    char* c = static_cast<char*>(p);
    e.base = p;
    e.bytes = bytes;
    e.d.off = reinterpret_cast<uint64_t*>(c);
    e.d.idx = reinterpret_cast<uint64_t*>(c + part[0]);
    e.d.val = rs->valued ? reinterpret_cast<float*>(c + part[0] + part[1]) : nullptr;
    e.d.lab = reinterpret_cast<float*>(c + part[0] + part[1] + part[2]);
    e.d.wt = rs->weighted ? reinterpret_cast<float*>(c + part[0] + part[1] + part[2] + part[3])
                          : nullptr;
  }
  rs->cap = cap;
  return 1;
}

// the ring regrown when an epoch's largest batch needs more than an entry holds -> *rc = 1;
// no longer inside the budget -> *rc = 0 (no ring left)
int ring_fit(dfx_reshuffle* rs, int64_t need, int* rc) {
  *rc = 1;
  if (need <= rs->cap) return DFX_OK;
  // the steps that read the ring must be past the device (the copies are: the epoch's wait)
  for (auto& e : rs->ring) DFX_HIP(hipEventSynchronize(e.consumed));
  ring_free(rs);
  *rc = ring_alloc(rs, std::min(rs->total_nnz, need + need / 4));
  return *rc < 0 ? DFX_ERR_HIP : DFX_OK;
}

void rs_release(dfx_reshuffle* rs) {
  ring_free(rs);
  for (auto& e : rs->ring)
    if (e.consumed) (void)hipEventDestroy(e.consumed);
  if (rs->scratch) batchcache_give(rs->bc, rs->scratch, rs->scratch_bytes);
  if (rs->samp) batchcache_give(rs->bc, rs->samp, rs->samp_bytes);
  if (rs->h_bnnz) (void)hipHostFree(rs->h_bnnz);
  if (rs->ev_epoch) (void)hipEventDestroy(rs->ev_epoch);
  delete rs;
}
}  // namespace

extern "C" int dfx_reshuffle_create(dfx_batchcache* bc, int64_t list, int64_t batch_rows,
                                    int nring, dfx_reshuffle** out, int* kept) {
  DFX_CHECK_ARG(bc && out && kept, "reshuffle_create: null argument");
  DFX_CHECK_ARG(batch_rows > 0, "reshuffle_create: batch_rows must be > 0");
  DFX_CHECK_ARG(nring >= 2 && nring <= 8, "reshuffle_create: nring must be in 2..8");
  *out = nullptr;
  *kept = 0;
  dfx_ctx* ctx = batchcache_ctx(bc);
  DFX_HIP(hipSetDevice(ctx->c.device));
  const dfx_batch* batches = nullptr;
  int64_t nb = 0;
  DFX_TRY(batchcache_sealed(bc, list, &batches, &nb));
  int64_t N = 0, nnz = 0;
  for (int64_t b = 0; b < nb; ++b) {
    N += batches[b].size;
    nnz += batches[b].nnz;
    DFX_CHECK_ARG(N < (1ll << 31), "reshuffle_create: the list holds 2^31 rows or more");
  }
  DFX_CHECK_ARG(nb < (1ll << 31), "reshuffle_create: the list holds 2^31 batches or more");
  dfx_reshuffle* rs = new dfx_reshuffle();
  rs->bc = bc;
  rs->ctx = ctx;
  rs->N = N;
  rs->R = N > 0 ? std::min(batch_rows, N) : 1;
  rs->nb_src = nb;
  rs->nb_out = (N + rs->R - 1) / rs->R;
  rs->total_nnz = nnz;
  rs->h_src.resize((size_t)nb);
  rs->h_prefix.assign((size_t)nb + 1, 0u);
  for (int64_t b = 0; b < nb; ++b) {
    const dfx_batch& s = batches[b];
    rs->h_src[(size_t)b] = RsSrc{s.offset, s.index, s.value, s.label, s.weight};
    rs->h_prefix[(size_t)b + 1] = rs->h_prefix[(size_t)b] + (uint32_t)s.size;
    rs->valued = rs->valued || s.value;
    rs->weighted = rs->weighted || s.weight;
  }
  rs->ring.resize((size_t)nring);
  // the table and the scratch, then the ring; what does not fit is given back
  const int64_t part[4] = {round_up(nb * (int64_t)sizeof(RsSrc)), round_up((nb + 1) * 4),
                           round_up(N * 4), round_up(N * 8)};
  rs->scratch_bytes = part[0] + part[1] + part[2] + part[3];
  int rc = batchcache_take(bc, rs->scratch_bytes, &rs->scratch);
  if (rc == 1) {
    // 1.25 times the mean batch, the whole list at most
    const int64_t mean = N > 0 ? (nnz / N + 1) * rs->R : 0;
    rc = ring_alloc(rs, std::max<int64_t>(std::min(nnz, mean + mean / 4), 64));
  } else {
    rs->scratch = nullptr;
  }
  if (rc != 1) {
    rs_release(rs);
    return rc < 0 ? DFX_ERR_HIP : DFX_OK;  // over the budget: *kept = 0, the cache untouched
  }
  char* c = static_cast<char*>(rs->scratch);
  rs->d_src = reinterpret_cast<RsSrc*>(c);
  rs->d_prefix = reinterpret_cast<uint32_t*>(c + part[0]);
  rs->d_len = reinterpret_cast<uint32_t*>(c + part[0] + part[1]);
  rs->d_ex = reinterpret_cast<uint64_t*>(c + part[0] + part[1] + part[2]);
  auto fail = [&](const char* what) {
    set_error(std::string("reshuffle_create: ") + what);
    rs_release(rs);
    return DFX_ERR_HIP;
  };
  for (auto& e : rs->ring)
    if (hipEventCreateWithFlags(&e.consumed, hipEventDisableTiming) != hipSuccess)
      return fail("event");
  if (hipEventCreateWithFlags(&rs->ev_epoch, hipEventDisableTiming) != hipSuccess)
    return fail("event");
  if (hipHostMalloc(reinterpret_cast<void**>(&rs->h_bnnz),
                    (size_t)(rs->nb_out + 1) * 8, hipHostMallocDefault) != hipSuccess)
    return fail("pinned counts");
  const hipStream_t st = in_stream(rs);
  if ((nb > 0 && hipMemcpyAsync(rs->d_src, rs->h_src.data(), (size_t)nb * sizeof(RsSrc),
                                hipMemcpyHostToDevice, st) != hipSuccess) ||
      hipMemcpyAsync(rs->d_prefix, rs->h_prefix.data(), (size_t)(nb + 1) * 4,
                     hipMemcpyHostToDevice, st) != hipSuccess)
    return fail("table upload");
  // joined here, once: the input stream may be another one by the first epoch
  if (hipStreamSynchronize(st) != hipSuccess) return fail("table upload");
  batchcache_hold(bc, +1);
  *out = rs;
  *kept = 1;
  return DFX_OK;
}

extern "C" int dfx_reshuffle_destroy(dfx_reshuffle* rs) {
  if (!rs) return DFX_OK;
  // queued copies write the ring, queued steps read it
  (void)hipSetDevice(rs->ctx->c.device);
  (void)hipDeviceSynchronize();
  batchcache_hold(rs->bc, -1);
  rs_release(rs);
  return DFX_OK;
}

extern "C" int dfx_reshuffle_begin_epoch(dfx_reshuffle* rs, uint64_t key, int64_t* n_batches) {
  DFX_CHECK_ARG(rs && n_batches, "reshuffle_begin_epoch: null argument");
  DFX_HIP(hipSetDevice(rs->ctx->c.device));
  rs->epoch_open = false;
  rs->handed = -1;
  rs->pos = 0;
  rs->sampled = false;
  rs->n_cur = rs->N;
  rs->nb_cur = rs->nb_out;
  rs->net = rs_make((uint32_t)rs->N, key);
  if (rs->N == 0) {
    rs->epoch_open = true;
    *n_batches = 0;
    return DFX_OK;
  }
  const hipStream_t st = in_stream(rs);
  const uint32_t n = (uint32_t)rs->N, nb = (uint32_t)rs->nb_src;
  hipLaunchKernelGGL(k_rs_len, dim3((unsigned)((rs->N + kNT - 1) / kNT)), dim3(kNT), 0, st,
                     rs->net, (const RsSrc*)rs->d_src, (const uint32_t*)rs->d_prefix, nb,
                     rs->d_len);
  hipLaunchKernelGGL(k_rs_scan, dim3((unsigned)rs->nb_out), dim3(kNT), 0, st,
                     (const uint32_t*)rs->d_len, n, (uint32_t)rs->R, rs->d_ex, rs->h_bnnz);
  DFX_HIP(hipGetLastError());
  DFX_HIP(hipEventRecord(rs->ev_epoch, st));
  DFX_HIP(hipEventSynchronize(rs->ev_epoch));  // the epoch's one host wait
  const volatile unsigned long long* h = rs->h_bnnz;
  int64_t need = 0, sum = 0;
  for (int64_t k = 0; k < rs->nb_out; ++k) {
    need = std::max<int64_t>(need, (int64_t)h[k]);
    sum += (int64_t)h[k];
  }
  if (sum != rs->total_nnz) {
    set_error("reshuffle_begin_epoch: the batches' nnz do not add up to the list's");
    return DFX_ERR_CHECK;
  }
  int rc = 1;
  DFX_TRY(ring_fit(rs, need, &rc));
  if (rc == 0) {  // no longer inside the budget: the caller replays the list as recorded
    *n_batches = -1;
    return DFX_OK;
  }
  rs->epoch_open = true;
  *n_batches = rs->nb_out;
  return DFX_OK;
}

extern "C" int dfx_reshuffle_begin_epoch_sampled(dfx_reshuffle* rs, uint64_t key,
                                                 float neg_sampling, int64_t* n_batches,
                                                 int64_t* n_rows) {
  DFX_CHECK_ARG(rs && n_batches && n_rows, "reshuffle_begin_epoch_sampled: null argument");
  DFX_CHECK_ARG(neg_sampling >= 0.f,  // (false for a NaN)
                "reshuffle_begin_epoch_sampled: neg_sampling must be a number >= 0");
  DFX_HIP(hipSetDevice(rs->ctx->c.device));
  rs->epoch_open = false;
  rs->handed = -1;
  rs->pos = 0;
  rs->sampled = true;
  rs->n_cur = rs->nb_cur = 0;
  rs->net = rs_make((uint32_t)rs->N, key);
  *n_rows = 0;
  if (rs->N == 0) {
    rs->epoch_open = true;
    *n_batches = 0;
    return DFX_OK;
  }
  const int64_t nt = (rs->N + kTile - 1) / kTile;
  if (!rs->samp) {
    const int64_t part[3] = {round_up(rs->N * 4), round_up(rs->N * 4), round_up((nt + 1) * 4)};
    const int64_t bytes = part[0] + part[1] + part[2];
    void* p = nullptr;
    const int rc = batchcache_take(rs->bc, bytes, &p);
    if (rc < 0) return DFX_ERR_HIP;
    if (rc == 0) {  // over the budget: nothing taken, nothing queued
      *n_batches = -1;
      return DFX_OK;
    }
    char* c = static_cast<char*>(p);
    rs->samp = p;
    rs->samp_bytes = bytes;
    rs->d_ksrc = reinterpret_cast<uint32_t*>(c);
    rs->d_klen = reinterpret_cast<uint32_t*>(c + part[0]);
    rs->d_tile = reinterpret_cast<uint32_t*>(c + part[0] + part[1]);
  }
  const hipStream_t st = in_stream(rs);
  const uint32_t n = (uint32_t)rs->N, nb = (uint32_t)rs->nb_src;
  // (d_ex is free until k_rs_scan_k writes it: its first 4 N bytes hold the flagged sources)
  uint32_t* flagged = reinterpret_cast<uint32_t*>(rs->d_ex);
  unsigned long long* hK = rs->h_bnnz + rs->nb_out;
  hipLaunchKernelGGL(k_rs_keep, dim3((unsigned)nt), dim3(kNT), 0, st, rs->net, key, neg_sampling,
                     (const RsSrc*)rs->d_src, (const uint32_t*)rs->d_prefix, nb, rs->d_len,
                     flagged, rs->d_tile);
  hipLaunchKernelGGL(k_rs_tiles, dim3(1), dim3(kNT), 0, st, rs->d_tile, (uint32_t)nt, hK);
  hipLaunchKernelGGL(k_rs_compact, dim3((unsigned)nt), dim3(kNT), 0, st,
                     (const uint32_t*)flagged, (const uint32_t*)rs->d_len, n,
                     (const uint32_t*)rs->d_tile, rs->d_ksrc, rs->d_klen);
  hipLaunchKernelGGL(k_rs_scan_k, dim3((unsigned)rs->nb_out), dim3(kNT), 0, st,
                     (const uint32_t*)rs->d_klen, (const uint32_t*)(rs->d_tile + nt),
                     (uint32_t)rs->R, rs->d_ex, rs->h_bnnz);
  DFX_HIP(hipGetLastError());
  DFX_HIP(hipEventRecord(rs->ev_epoch, st));
  DFX_HIP(hipEventSynchronize(rs->ev_epoch));  // the epoch's one host wait
  const volatile unsigned long long* h = rs->h_bnnz;
  const int64_t K = (int64_t)h[rs->nb_out], nbk = (K + rs->R - 1) / rs->R;
  int64_t need = 0, sum = 0;
  for (int64_t k = 0; k < nbk; ++k) {
    need = std::max<int64_t>(need, (int64_t)h[k]);
    sum += (int64_t)h[k];
  }
  if (K > rs->N || sum > rs->total_nnz) {
    set_error("reshuffle_begin_epoch_sampled: more rows or ids kept than the list holds");
    return DFX_ERR_CHECK;
  }
  int rc = 1;
  DFX_TRY(ring_fit(rs, need, &rc));
  if (rc == 0) {
    *n_batches = -1;
    return DFX_OK;
  }
  rs->n_cur = K;
  rs->nb_cur = nbk;
  rs->epoch_open = true;
  *n_batches = nbk;
  *n_rows = K;
  return DFX_OK;
}

extern "C" int dfx_reshuffle_next(dfx_reshuffle* rs, dfx_batch* batch, int* has) {
  DFX_CHECK_ARG(rs && batch && has, "reshuffle_next: null argument");
  DFX_CHECK_ARG(rs->epoch_open, "reshuffle_next: no epoch begun (dfx_reshuffle_begin_epoch)");
  *has = 0;
  if (rs->pos >= rs->nb_cur) return DFX_OK;
  DFX_HIP(hipSetDevice(rs->ctx->c.device));
  const int slot = (int)(rs->pos % (int64_t)rs->ring.size());
  auto& e = rs->ring[(size_t)slot];
  const int64_t j0 = rs->pos * rs->R, rows = std::min(rs->R, rs->n_cur - j0);
  const int64_t nnz = (int64_t)rs->h_bnnz[rs->pos];
  if (nnz > rs->cap) {
    set_error("reshuffle_next: a batch larger than the ring entry");
    return DFX_ERR_CHECK;
  }
  const hipStream_t st = in_stream(rs);
  // the step that took this entry a round ago must be past the device: a stream wait
  DFX_HIP(hipStreamWaitEvent(st, e.consumed, 0));
  const dim3 grid((unsigned)((rows + kWavesPerBlock - 1) / kWavesPerBlock));
  if (rs->sampled)
    hipLaunchKernelGGL(k_rs_copy_k, grid, dim3(kNT), 0, st, (const uint32_t*)rs->d_ksrc,
                       (const RsSrc*)rs->d_src, (const uint32_t*)rs->d_prefix,
                       (uint32_t)rs->nb_src, (const uint64_t*)rs->d_ex, (uint32_t)j0,
                       (uint32_t)rows, e.d);
  else
    hipLaunchKernelGGL(k_rs_copy, grid, dim3(kNT), 0, st, rs->net, (const RsSrc*)rs->d_src,
                       (const uint32_t*)rs->d_prefix, (uint32_t)rs->nb_src,
                       (const uint64_t*)rs->d_ex, (uint32_t)j0, (uint32_t)rows, e.d);
  DFX_HIP(hipGetLastError());
  *batch = dfx_batch{};
  batch->size = rows;
  batch->nnz = nnz;
  batch->offset = e.d.off;
  batch->index = e.d.idx;
  batch->value = e.d.val;
  batch->label = e.d.lab;
  batch->weight = e.d.wt;
  rs->handed = slot;
  rs->pos += 1;
  *has = 1;
  return DFX_OK;
}

extern "C" int dfx_reshuffle_consumed(dfx_reshuffle* rs) {
  DFX_CHECK_ARG(rs, "reshuffle_consumed: null argument");
  DFX_CHECK_ARG(rs->handed >= 0, "reshuffle_consumed: no batch handed out");
  DFX_HIP(hipEventRecord(rs->ring[(size_t)rs->handed].consumed, rs->ctx->c.stream));
  rs->handed = -1;
  return DFX_OK;
}

extern "C" int dfx_reshuffle_stats(dfx_reshuffle* rs, int64_t* out) {
  DFX_CHECK_ARG(rs && out, "reshuffle_stats: null argument");
  out[0] = rs->N;
  out[1] = rs->nb_out;
  out[2] = 0;
  for (const auto& e : rs->ring) out[2] += e.bytes;
  out[3] = rs->scratch_bytes + rs->samp_bytes;
  return DFX_OK;
}
